"""ctypes loader for libdistance_hip.so (the C ABI in include/distance_hip.h).

There is no CPU fallback and no torch dependency here: if the HIP library is missing this module
raises, and every device call fails with a DistanceError when HIP does.
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DST_LIB_PATH") or os.path.join(_HERE, "libdistance_hip.so")   # DST_LIB_PATH: measurement builds (tools/variants.sh)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "distance_hip.h")

_u8p = C.POINTER(C.c_uint8)
_u32p = C.POINTER(C.c_uint32)
_u64p = C.POINTER(C.c_uint64)
_vp = C.c_void_p
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
SLAB_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p)
# dst_links_sink(user, first_link, n_links, row, col, values, tallies)
LINKS_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
LINKS_VALUES, LINKS_TALLIES = 1, 2
LINKS_CHUNK = 1 << 22   # DST_LINKS_CHUNK: the most links of one sink call
# dst_ld_sink(user, first_link, n_links, pos_i, pos_j, tallies)
LD_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p)
LD_CHUNK = 1 << 22      # DST_LD_CHUNK: the most links of one dst_ld_sink call
LD_SCALE_BITS = 30      # DST_LD_SCALE_BITS: a decay bin sums r2 as rint(r2 * 2^30)
LD_DECAY_MAX_BINS = 4096    # DST_LD_DECAY_MAX_BINS
LD_DECAY_LOCAL_BINS = 512   # DST_LD_DECAY_LOCAL_BINS: a tile spanning at most this many bins accumulates on chip
STREAM_LINKS_WINDOW = 1 << 20   # DST_STREAM_LINKS_WINDOW: the default most links of one window of a links stream
PAIR_SITES_BATCH = 1 << 20    # DST_PAIR_SITES_BATCH: the most pairs of one device batch of dst_pair_sites
PAIR_SITES_WINDOW = 1 << 24   # DST_PAIR_SITES_WINDOW: the most entries of one device output window
RUN_PAIRS_BATCH = 1 << 20     # DST_RUN_PAIRS_BATCH: the most pairs of one device batch of dst_run_pairs
PAIRS_AUTO, PAIRS_DIRECT, PAIRS_SWEEP = 0, 1, 2   # DST_PAIRS_*: the routes of dst_run_pairs
WINDOWS_MAX = 65536           # DST_WINDOWS_MAX: the most windows of one dst_run_windows call
SUMMARY_SCALE_BITS = 37  # DST_SUMMARY_SCALE_BITS: f64 distances are summed as rint(v * 2^37)
SUMMARY_MAX_BINS = 4096   # DST_SUMMARY_MAX_BINS
STREAM_SUMMARY_LOADED, STREAM_SUMMARY_STREAMED = 1, 2   # DST_STREAM_SUMMARY_*: the sides of a summary stream
STREAM_SUMMARY_ROWS = 64     # kStreamSummaryRows (csrc/dst_internal.h): the tile of a summary stream's kernel, streamed records
STREAM_SUMMARY_COLS = 256    # kStreamSummaryCols: ... and loaded records
STREAM_GROUPS_LOADED, STREAM_GROUPS_STREAMED = 1, 2   # DST_STREAM_GROUPS_*: the tables of a group-summary stream
STREAM_GROUPS_ROWS = 64      # kStreamGroupRows (csrc/dst_internal.h): the tile of a group-summary stream's column kernel, streamed records
STREAM_GROUPS_COLS = 256     # kStreamGroupCols: ... and loaded records
GROUPS_MAX = 1024         # DST_GROUPS_MAX: the most groups of one side of dst_group_summary
WINDOW_GROUPS_MAX = 256   # DST_WINDOW_GROUPS_MAX: the most groups of one side of dst_window_group_summary
GROUP_NONE = 0xFFFFFFFF   # DST_GROUP_NONE: a record that belongs to no group
SITE_CLASSES = 5          # DST_SITE_CLASSES: A, T, G, C, ambiguous of a dst_site_counts entry
SITE_FLUSH_PERIOD = 15    # DST_SITE_FLUSH_PERIOD: records a thread of the site-count kernel takes before it adds to the counts
SITE_STRIP_RECORDS = 3840   # DST_SITE_STRIP_RECORDS: records of one group a workgroup of that kernel counts


class LaunchInfo(C.Structure):
    """dst_launch_info"""
    _fields_ = [("path", C.c_int), ("measure", C.c_int), ("family", C.c_int), ("out_kind", C.c_int), ("wide", C.c_int),
                ("square", C.c_int), ("event_waves", C.c_int), ("heavy_events", C.c_int), ("rows_per_tile", C.c_uint32),
                ("tile_cols", C.c_uint32), ("tiles", C.c_uint64), ("hot", C.c_int), ("run_records", C.c_int),
                ("variant", C.c_int), ("ksplit", C.c_uint32), ("pairs", C.c_uint64), ("events_per_pair", C.c_double),
                ("list_length", C.c_double), ("run_adds", C.c_double)]


class LdBin(C.Structure):
    """dst_ld_bin"""
    _fields_ = [("pairs", C.c_uint64), ("defined", C.c_uint64), ("links", C.c_uint64), ("r2_sum", C.c_double)]


class SummaryTotals(C.Structure):
    """dst_summary_totals"""
    _fields_ = [("pairs", C.c_uint64), ("nan_pairs", C.c_uint64), ("summable_pairs", C.c_uint64), ("links", C.c_uint64),
                ("sum", C.c_double)]


class GroupCell(C.Structure):
    """dst_group_cell"""
    _fields_ = [("pairs", C.c_uint64), ("nan_pairs", C.c_uint64), ("summable_pairs", C.c_uint64), ("links", C.c_uint64),
                ("sum", C.c_double), ("min_bits", C.c_uint64), ("max_bits", C.c_uint64)]


class SiteWindow(C.Structure):
    """dst_site_window"""
    _fields_ = [("records", C.c_uint64), ("sites", C.c_uint64), ("called", C.c_uint64), ("segregating", C.c_uint64),
                ("theta_sum", C.c_double), ("pi_sum", C.c_double)]


class PairsInfo(C.Structure):
    """dst_pairs_info"""
    _fields_ = [("route", C.c_int), ("lanes_per_pair", C.c_uint32), ("direct_pairs", C.c_uint64), ("swept_pairs", C.c_uint64),
                ("slabs", C.c_uint64)]


class DistanceError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"[dst status {status}] {message}")
        self.status = status
        self.message = message


def declared_symbols() -> list[str]:
    """Every function include/distance_hip.h declares (used by the CPU symbol-export test)."""
    text = open(HEADER_PATH).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dst_[a-z0-9_]+)\s*\(", text)))


_SIGS = {
    "dst_abi_version": (C.c_int, []),
    "dst_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "dst_measure_from_name": (C.c_int, [C.c_char_p]),
    "dst_tally_width": (C.c_int, [C.c_int]),
    "dst_status_string": (C.c_char_p, [C.c_int]),
    "dst_build_flags": (C.c_char_p, []),
    "dst_create": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "dst_destroy": (C.c_int, [_vp]),
    "dst_last_error": (C.c_char_p, [_vp]),
    "dst_set_variant": (C.c_int, [_vp, C.c_int]),
    "dst_variant_count": (C.c_int, [C.c_int]),
    "dst_set_ksplit": (C.c_int, [_vp, C.c_int]),
    "dst_set_path": (C.c_int, [_vp, C.c_int]),
    "dst_last_path": (C.c_int, [_vp]),
    "dst_last_launch": (C.c_int, [_vp, _vp]),
    "dst_plan_consensus_launch": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64,
                                            C.c_double, C.c_double, C.c_double, C.c_int, _vp]),
    "dst_run_records": (C.c_int, [_vp, C.c_int, _u64p, _u64p]),
    "dst_planes_stored": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_int)]),
    "dst_consensus": (C.c_int, [_vp, C.c_int, _vp, C.c_size_t]),
    "dst_differences": (C.c_int, [_vp, C.c_int, _vp, C.c_size_t, _vp, _vp, C.c_size_t, _u64p]),
    "dst_site_tallies": (C.c_int, [C.c_int, C.c_uint8, C.c_uint8, C.POINTER(C.c_int)]),
    "dst_upload": (C.c_int, [_vp, C.c_int, _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp]),
    "dst_upload_device": (C.c_int, [_vp, C.c_int, _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp, _vp]),
    "dst_set_info": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "dst_get_base_counts": (C.c_int, [_vp, C.c_int, _vp]),
    "dst_square_pairs": (C.c_uint64, [C.c_uint64]),
    "dst_square_row_start": (C.c_uint64, [C.c_uint64, C.c_uint64]),
    "dst_partition_square": (C.c_int, [C.c_uint64, C.c_int, _u64p]),
    "dst_partition_rect": (C.c_int, [C.c_uint64, C.c_int, _u64p]),
    "dst_run_square": (C.c_int, [_vp, C.c_int, C.c_uint64, C.c_uint64, C.c_int, _vp, C.c_size_t, _vp]),
    "dst_run_rect": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_int, _vp,
                               C.c_size_t, _vp]),
    "dst_finalize_device": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_int,
                                      _vp, _vp, C.c_size_t, _vp]),
    "dst_run_square_host": (C.c_int, [_vp, C.c_int, C.c_uint64, C.c_uint64, C.c_int, _vp, C.c_size_t]),
    "dst_run_rect_host": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_int, _vp,
                                    C.c_size_t]),
    "dst_run_slabs": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, _vp, _vp]),
    "dst_stream_open": (C.c_int, [_vp, C.c_int, C.c_int, C.c_size_t, C.c_int, C.POINTER(_vp)]),
    "dst_stream_open_wire": (C.c_int, [_vp, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, C.POINTER(_vp)]),
    "dst_stream_acquire": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_size_t), C.POINTER(_vp)]),
    "dst_stream_submit": (C.c_int, [_vp, C.c_size_t, C.c_int]),
    "dst_stream_collect": (C.c_int, [_vp, C.POINTER(C.c_size_t), C.POINTER(_vp)]),
    "dst_stream_in_flight": (C.c_int, [_vp]),
    "dst_stream_close": (C.c_int, [_vp]),
    "dst_stream_open_closest": (C.c_int, [_vp, C.c_int, C.c_uint32, C.c_int, C.c_size_t, C.c_int, C.c_int, C.POINTER(_vp)]),
    "dst_stream_closest_next_index": (C.c_int, [_vp, C.c_uint64]),
    "dst_stream_closest_result": (C.c_int, [_vp, _vp, _vp, _vp, C.c_size_t, _u32p]),
    "dst_stream_closest_batch": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), _u32p]),
    "dst_stream_open_links": (C.c_int, [_vp, C.c_int, C.c_double, C.c_int, C.c_uint64, C.c_size_t, C.c_int, C.c_int, C.POINTER(_vp)]),
    "dst_stream_links_batch": (C.c_int, [_vp, C.c_uint64, _u64p, _u64p, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "dst_stream_links_stats": (C.c_int, [_vp, _u64p, _u64p]),
    "dst_stream_open_window_closest": (C.c_int, [_vp, C.c_int, C.c_uint32, _vp, _vp, C.c_uint32, C.c_uint64, C.c_size_t, C.c_int,
                                                 C.c_int, C.POINTER(_vp)]),
    "dst_stream_window_closest_result": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_size_t, _u32p]),
    "dst_comm_unique_id": (C.c_int, [_vp, C.c_size_t]),
    "dst_comm_create": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.POINTER(_vp)]),
    "dst_comm_create_custom": (C.c_int, [_vp, C.c_int, C.c_int, ALLGATHER_FN, _vp, C.POINTER(_vp)]),
    "dst_comm_destroy": (C.c_int, [_vp]),
    "dst_upload_shared": (C.c_int, [_vp, C.c_int, _vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, _vp]),
    "dst_shared_range": (C.c_int, [C.c_uint64, C.c_int, C.c_int, _u64p, _u64p]),
    "dst_shared_block_layout": (C.c_int, [C.c_uint64, C.c_int, C.c_uint32, _u32p]),
    "dst_shared_stats": (C.c_int, [_vp, C.c_int, _u64p, _u64p, _u64p]),
    "dst_comm_info": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "dst_gather_slabs": (C.c_int, [_vp, _vp, _vp, _u64p, _u64p, C.c_int, _vp]),
    "dst_nearest": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, _vp, _vp, _vp, C.c_size_t, _u32p]),
    "dst_clusters": (C.c_int, [_vp, C.c_int, C.c_double, C.c_uint64, _vp, C.c_size_t, _u64p, _u64p]),
    "dst_representatives": (C.c_int, [_vp, C.c_int, C.c_double, C.c_uint64, _vp, _vp, _vp, C.c_size_t, _u64p]),
    "dst_links": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_uint64, C.c_int, _vp, _vp, _u64p]),
    "dst_pair_sites": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_uint64, _vp, _vp, _vp, C.c_size_t, _u64p]),
    "dst_run_pairs": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_uint64, C.c_int, C.c_uint64, _vp, _vp,
                                C.c_size_t, _vp]),
    "dst_run_pairs_lanes": (C.c_uint32, [C.c_uint64]),
    "dst_run_windows": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, _vp, _vp, C.c_uint32, C.c_int,
                                  _vp, C.c_size_t, _vp]),
    "dst_run_windows_host": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, _vp, _vp, C.c_uint32,
                                       C.c_int, _vp, C.c_size_t]),
    "dst_window_base_counts": (C.c_int, [_vp, C.c_int, _vp, _vp, C.c_uint32, _vp, C.c_size_t]),
    "dst_nearest_windows": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, _vp, _vp, C.c_uint32,
                                      C.c_uint32, C.c_uint64, _vp, _vp, _vp, C.c_size_t, _u32p]),
    "dst_sliding_windows": (C.c_int, [C.c_uint64, C.c_uint64, C.c_uint64, _vp, _vp, C.c_size_t, _u32p]),
    "dst_summary": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_uint64, C.c_uint32, C.c_double, _vp, _vp,
                              _vp, _vp, C.c_size_t, _vp]),
    "dst_stream_open_summary": (C.c_int, [_vp, C.c_int, C.c_double, C.c_int, C.c_uint32, C.c_double, C.c_size_t, C.c_int, C.c_int,
                                          C.POINTER(_vp)]),
    "dst_stream_summary_batch": (C.c_int, [_vp, C.POINTER(C.c_size_t), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "dst_stream_summary_result": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp, _u64p]),
    "dst_stream_open_group_summary": (C.c_int, [_vp, C.c_int, C.c_double, C.c_int, _vp, C.c_uint32, C.c_uint32, C.c_size_t, C.c_int,
                                                C.c_int, C.POINTER(_vp)]),
    "dst_stream_group_labels": (C.c_int, [_vp, C.POINTER(_vp)]),
    "dst_stream_group_summary_batch": (C.c_int, [_vp, C.POINTER(C.c_size_t), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "dst_stream_group_summary_result": (C.c_int, [_vp, _vp, C.c_size_t, _vp, _vp, _vp, C.c_size_t, _u64p]),
    "dst_window_summary": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_uint32, C.c_double, _vp, _vp, _vp,
                                     _vp, C.c_size_t]),
    "dst_group_summary": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_uint32, _vp, C.c_uint32, C.c_double,
                                    C.c_uint64, _vp, C.c_size_t, _vp, _vp, _vp, C.c_size_t]),
    "dst_window_group_summary": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_uint32, _vp, C.c_uint32, _vp,
                                           C.c_uint32, C.c_double, _vp, C.c_size_t, _vp, _vp, _vp, C.c_size_t]),
    "dst_site_counts": (C.c_int, [_vp, C.c_int, _vp, C.c_uint32, C.c_uint64, C.c_uint64, _vp, C.c_size_t]),
    "dst_site_stats": (C.c_int, [_vp, C.c_uint64, C.c_uint64, C.c_uint32, _vp, _vp, C.c_uint32, _vp, _vp, C.c_size_t]),
    "dst_site_ld": (C.c_int, [_vp, C.c_int, _vp, _vp, C.c_uint32, _vp, C.c_uint32, C.c_uint32, C.c_uint32, _vp, C.c_size_t]),
    "dst_site_ld_links": (C.c_int, [_vp, C.c_int, _vp, _vp, C.c_uint32, _vp, C.c_uint32, C.c_double, C.c_uint64, _vp, _vp, _u64p]),
    "dst_ld_band": (C.c_int, [_vp, C.c_uint32, C.c_uint64, _vp, _u64p, _u64p]),
    "dst_site_ld_band": (C.c_int, [_vp, C.c_int, _vp, _vp, C.c_uint32, _vp, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, _vp, C.c_size_t]),
    "dst_site_ld_links_band": (C.c_int, [_vp, C.c_int, _vp, _vp, C.c_uint32, _vp, C.c_uint32, C.c_double, C.c_uint64, C.c_uint64, _vp, _vp,
                                         _u64p]),
    "dst_site_ld_decay": (C.c_int, [_vp, C.c_int, _vp, _vp, C.c_uint32, _vp, C.c_uint32, C.c_double, C.c_uint64, C.c_uint32, C.c_uint64,
                                    _vp, C.c_size_t]),
    "dst_ld_finalize": (C.c_int, [_vp, C.c_uint64, _vp, _vp, _vp]),
    "dst_site_major": (C.c_int, [_vp, C.c_uint64, C.c_uint32, C.c_uint32, _vp, _vp, _vp]),
    "dst_mst": (C.c_int, [_vp, C.c_int, C.c_uint64, _vp, _vp, _vp, _vp, C.c_size_t, _u64p, _u32p]),
    "dst_nj": (C.c_int, [_vp, C.c_int, C.c_uint64, _vp, _vp, C.c_size_t]),
    "dst_nj_matrix": (C.c_int, [_vp, _vp, C.c_uint64, _vp, _vp, C.c_size_t]),
    "dst_newick": (C.c_int, [C.c_uint64, _vp, _vp, C.c_char_p, _vp, _vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "dst_newick_support": (C.c_int, [C.c_uint64, _vp, _vp, C.c_char_p, _vp, _vp, _vp, C.c_size_t,
                                     C.POINTER(C.c_size_t)]),
    "dst_dendrogram": (C.c_int, [_vp, C.c_int, C.c_int, C.c_uint64, _vp, _vp, _vp, C.c_size_t, _u64p]),
    "dst_dendrogram_matrix": (C.c_int, [_vp, _vp, C.c_uint64, C.c_int, _vp, _vp, _vp, C.c_size_t, _u64p]),
    "dst_newick_rooted": (C.c_int, [C.c_uint64, _vp, _vp, C.c_char_p, _vp, _vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "dst_bootstrap_columns": (None, [C.c_uint64, C.c_uint32, C.c_uint64, _vp]),
    "dst_nj_bootstrap": (C.c_int, [_vp, C.c_int, _vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_uint32, C.c_uint64,
                                   C.c_uint64, _vp, _vp, _vp, C.c_size_t]),
    "dst_host_alloc": (C.c_int, [C.c_size_t, C.POINTER(_vp)]),
    "dst_host_free": (C.c_int, [_vp]),
    "dst_out_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_uint64]),
    "dst_kernel_ms_mean": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "dst_last_kernel_ms": (C.c_int, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "dst_plan_tiles": (C.c_int, [C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_int, _vp,
                                 C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "dst_finalize": (C.c_int, [C.c_int, _vp, _vp, _vp, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "dst_format_distance": (C.c_int, [C.c_int, C.c_double, C.c_int64, C.c_char_p, C.c_size_t]),
    "dst_set_prep_threshold": (C.c_int, [_vp, C.c_double]),
    "dst_set_ids": (C.c_int, [_vp, C.c_int, C.c_char_p, _u64p, C.c_uint64]),
    "dst_text_stats": (C.c_int, [_vp, _u64p, _u64p]),
    "dst_text_square": (C.c_int, [_vp, C.c_int, C.c_uint64, C.c_uint64, _vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "dst_text_rect": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_int, _vp, C.c_size_t,
                                C.POINTER(C.c_size_t)]),
    "dst_text_matrix": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_int, _vp,
                                  C.c_size_t, C.POINTER(C.c_size_t)]),
}

_lib = None


def load() -> C.CDLL:
    """Load the HIP library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  distance_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
