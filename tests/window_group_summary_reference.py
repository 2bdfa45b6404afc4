"""dst_window_group_summary's definition (include/distance_hip.h) for the tests: group_summary_reference.group_summary
applied to each window's full result (the context's own run_windows values, canonical order) and the labels, the answers
stacked window-major.  It gives what the library must return, to the bit.  It does not use distance_amd."""
import numpy as np

from group_summary_reference import CELL_KEYS, REC_KEYS, bits, check_consequences, group_summary

WINDOW_GROUPS_MAX = 256


def window_group_summary(measure, vals, n_rows, n_cols, square, threshold, row_group, n_row_groups, col_group=None,
                         n_col_groups=None):
    """The dict Engine.window_group_summary returns (per_record=True) from vals[n_windows, P], the per-window payloads."""
    vals = np.asarray(vals)
    assert vals.ndim == 2
    per = [group_summary(measure, v, n_rows, n_cols, square, threshold, row_group, n_row_groups, col_group, n_col_groups)
           for v in vals]
    return {k: np.stack([p[k] for p in per]) for k in CELL_KEYS + REC_KEYS}


def assert_window_group_summary(got, want, what=""):
    """integers equal, doubles bitwise; `got` may lack the per-record tables"""
    for k in CELL_KEYS + tuple(k for k in REC_KEYS if k in got):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].shape)
        assert np.array_equal(bits(got[k]), bits(want[k])), (what, k)


def check_window_consequences(res, row_group, square):
    """group_summary_reference.check_consequences inside every window"""
    for w in range(len(res["pairs"])):
        check_consequences({k: v[w] for k, v in res.items()}, row_group, square)
