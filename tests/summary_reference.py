"""dst_summary's definition (include/distance_hip.h) restated in numpy and Python integers, for the tests: applied to a full
result (the context's own run_square / run_rect values, canonical order) it gives what the library must return, to the
bit.  Sums are Python ints, converted once with float(int) (round to nearest even) and scaled with math.ldexp."""
import math

import numpy as np

from links_reference import INT_MEASURES, linked, pairs

SCALE_BITS = 37
LIMIT = 2.0 ** 25


def fixed_point(measure, vals):
    """(summable mask, q as int64, 0 where not summable): |q| < 2^62 for the f64 measures, so int64 holds it exactly"""
    vals = np.asarray(vals).reshape(-1)
    if measure in INT_MEASURES:
        return np.ones(len(vals), bool), vals.astype(np.int64)
    with np.errstate(invalid="ignore"):
        ok = np.abs(vals) < LIMIT   # (False for NaN)
    q = np.rint(np.where(ok, vals, 0.0) * 2.0 ** SCALE_BITS)   # the product is exact; rint rounds to nearest even
    return ok, q.astype(np.int64)


def width_q(measure, width):
    return int(width) if measure in INT_MEASURES else int(np.rint(width * 2.0 ** SCALE_BITS))


def bin_index(measure, vals, bins, width):
    """The bin of every value, -1 for NaN.  q and width_q are below 2^62 in magnitude: numpy's int64 floor_divide is the
    exact floor quotient."""
    vals = np.asarray(vals).reshape(-1)
    ok, q = fixed_point(measure, vals)
    wq = width_q(measure, width)
    assert 1 <= wq < 2 ** 62
    out = np.clip(np.floor_divide(q, np.int64(wq)), 0, bins - 1)
    if measure not in INT_MEASURES:
        with np.errstate(invalid="ignore"):
            out[~ok & (vals > 0)] = bins - 1   # v >= 2^25, +inf included
            out[~ok & (vals < 0)] = 0          # v <= -2^25
        out[np.isnan(vals)] = -1
    return out


def convert(measure, s):
    """the exact integer sum to double once, f64 measures scaled by 2^-37 (exact)"""
    d = float(s)
    return d if measure in INT_MEASURES else math.ldexp(d, -SCALE_BITS)


def summary(measure, vals, n_rows, n_cols, square, threshold, bins=0, width=1.0):
    """The dict Engine.summary returns (per_record=True), from the full result."""
    vals = np.asarray(vals).reshape(-1)
    i, j = pairs(n_rows, n_cols, square)
    assert len(vals) == len(i)
    link = linked(measure, vals, threshold)
    ok, q = fixed_point(measure, vals)
    nan = np.zeros(len(vals), bool) if measure in INT_MEASURES else np.isnan(vals)
    within = np.bincount(i[link], minlength=n_rows)
    summable = np.bincount(i[ok], minlength=n_rows)
    if square:
        within = within + np.bincount(j[link], minlength=n_rows)
        summable = summable + np.bincount(j[ok], minlength=n_rows)
    if int(np.abs(q).max(initial=0)) * max(len(q), 1) < 2 ** 62:
        # no int64 sum can overflow: numpy's integer sums are the exact sums
        q64 = q
        if square:
            full = np.zeros((n_rows, n_rows), np.int64)
            full[i, j] = q64
            full[j, i] = q64
        else:
            full = q64.reshape(n_rows, n_cols)
        sums = [int(x) for x in full.sum(axis=1, dtype=np.int64)]
        total = int(q64.sum(dtype=np.int64))
    else:
        sums, total = [0] * n_rows, 0
        for k in np.nonzero(ok)[0]:
            total += int(q[k])
            sums[i[k]] += int(q[k])
            if square:
                sums[j[k]] += int(q[k])
    out = {"within": within.astype(np.uint32), "summable": summable.astype(np.uint32),
           "sum": np.array([convert(measure, s) for s in sums], np.float64).reshape(n_rows),
           "pairs": len(vals), "nan_pairs": int(nan.sum()), "summable_pairs": int(ok.sum()), "links": int(link.sum()),
           "total_sum": convert(measure, total)}
    if bins:
        out["hist"] = hist_of(measure, vals, bins, width)
    return out


def hist_of(measure, vals, bins, width):
    b = bin_index(measure, vals, bins, width)
    return np.bincount(b[b >= 0], minlength=bins).astype(np.uint64)


def rethreshold(want, measure, vals, n_rows, n_cols, square, threshold):
    """`want` (a result of summary) at another threshold: only `within` and `links` depend on it."""
    vals = np.asarray(vals).reshape(-1)
    i, j = pairs(n_rows, n_cols, square)
    link = linked(measure, vals, threshold)
    within = np.bincount(i[link], minlength=n_rows)
    if square:
        within = within + np.bincount(j[link], minlength=n_rows)
    return dict(want, within=within.astype(np.uint32), links=int(link.sum()))


def assert_summary(got, want, what=""):
    """integers equal, sums bitwise"""
    for key in ("pairs", "nan_pairs", "summable_pairs", "links"):
        assert got[key] == want[key], (what, key, got[key], want[key])
    assert np.float64(got["total_sum"]).view(np.uint64) == np.float64(want["total_sum"]).view(np.uint64), (what, got["total_sum"], want["total_sum"])
    if "within" in got:
        assert got["within"].dtype == np.uint32 and got["summable"].dtype == np.uint32 and got["sum"].dtype == np.float64, what
        assert np.array_equal(got["within"], want["within"]), (what, "within")
        assert np.array_equal(got["summable"], want["summable"]), (what, "summable")
        assert np.array_equal(got["sum"].view(np.uint64), want["sum"].view(np.uint64)), (what, "sum")
    if "hist" in got:
        assert got["hist"].dtype == np.uint64 and np.array_equal(got["hist"], want["hist"]), (what, "hist")
        assert int(got["hist"].sum()) + got["nan_pairs"] == got["pairs"], what
