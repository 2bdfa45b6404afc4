"""dst_window_summary's definition (include/distance_hip.h) for the tests: summary_reference.summary applied to each
window's full result (the context's own run_windows values, canonical order), the answers stacked window-major.  It gives
what the library must return, to the bit.  It does not use distance_amd."""
import numpy as np

from summary_reference import summary

TOTALS = ("pairs", "nan_pairs", "summable_pairs", "links")


def window_summary(measure, vals, n_rows, n_cols, square, threshold):
    """The dict Engine.window_summary returns (per_record=True) from vals[n_windows, P], the per-window payloads."""
    vals = np.asarray(vals)
    assert vals.ndim == 2
    per = [summary(measure, v, n_rows, n_cols, square, threshold) for v in vals]
    nw = len(per)
    out = {k: np.array([p[k] for p in per], np.uint64).reshape(nw) for k in TOTALS}
    out["total_sum"] = np.array([p["total_sum"] for p in per], np.float64).reshape(nw)
    out["within"] = np.array([p["within"] for p in per], np.uint32).reshape(nw, n_rows)
    out["summable"] = np.array([p["summable"] for p in per], np.uint32).reshape(nw, n_rows)
    out["sum"] = np.array([p["sum"] for p in per], np.float64).reshape(nw, n_rows)
    return out


def assert_window_summary(got, want, what=""):
    """integers equal, sums by their bits; the per-record arrays when `got` has them"""
    for key in TOTALS:
        assert got[key].dtype == np.uint64 and got[key].shape == want[key].shape, (what, key)
        assert np.array_equal(got[key], want[key]), (what, key, got[key], want[key])
    assert got["total_sum"].dtype == np.float64 and got["total_sum"].shape == want["total_sum"].shape, what
    assert np.array_equal(got["total_sum"].view(np.uint64), want["total_sum"].view(np.uint64)), (what, "total_sum", got["total_sum"],
                                                                                                want["total_sum"])
    if "within" in got:
        assert got["within"].dtype == np.uint32 and got["summable"].dtype == np.uint32 and got["sum"].dtype == np.float64, what
        for key in ("within", "summable"):
            assert got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), (what, key)
        assert got["sum"].shape == want["sum"].shape, what
        assert np.array_equal(got["sum"].view(np.uint64), want["sum"].view(np.uint64)), (what, "sum")
