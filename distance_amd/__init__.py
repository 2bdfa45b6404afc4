"""distance_amd — MI355X-native all-pairs genetic distances (drop-in for the hot path of
benjamincjackson/distance: src/measures.rs + src/encoding.rs).

The product is ``libdistance_hip.so`` (hand-written gfx950 HIP kernels behind the C ABI of
``include/distance_hip.h``) plus the native CLI; this package is the thin Python host used by the
tests and ``bench.py``.  It never imports ``oracle`` and has no CPU compute path.
"""
from ._lib import LD_CHUNK, LD_DECAY_LOCAL_BINS, LD_DECAY_MAX_BINS, LD_SCALE_BITS, LD_SINK, LINKS_CHUNK, LINKS_SINK, PAIR_SITES_BATCH, PAIR_SITES_WINDOW, RUN_PAIRS_BATCH, SITE_CLASSES, SITE_FLUSH_PERIOD, SITE_STRIP_RECORDS, SUMMARY_MAX_BINS, SUMMARY_SCALE_BITS, WINDOWS_MAX, WINDOW_GROUPS_MAX, DistanceError, LIB_PATH, declared_symbols, load
from .engine import (OUT_DISTANCE, OUT_TALLY, OUT_TALLY16, FLOAT_MEASURES, INT_MEASURES, MEASURES, ClosestStream, Comm, Engine, GroupSummaryStream, LinksStream, SummaryStream, WindowClosestStream, bootstrap_columns, finalize, format_distance, ld_band, ld_finalize, newick, newick_rooted,
                     partition_rect, partition_square, plan_consensus_launch, plan_tiles, shared_range, site_major, site_stats, sliding_windows, square_pairs, square_row_start, tally_width)

__all__ = ["DistanceError", "Engine", "Comm", "ClosestStream", "GroupSummaryStream", "LinksStream", "SummaryStream", "WindowClosestStream", "shared_range", "MEASURES", "INT_MEASURES", "FLOAT_MEASURES", "LIB_PATH",
           "declared_symbols", "load", "LINKS_CHUNK", "LINKS_SINK", "PAIR_SITES_BATCH", "PAIR_SITES_WINDOW", "RUN_PAIRS_BATCH", "SUMMARY_MAX_BINS", "SUMMARY_SCALE_BITS", "bootstrap_columns", "finalize", "format_distance", "newick", "newick_rooted", "partition_square",
           "partition_rect", "plan_consensus_launch", "plan_tiles", "sliding_windows", "square_pairs", "square_row_start", "tally_width", "WINDOWS_MAX", "WINDOW_GROUPS_MAX", "site_stats", "SITE_CLASSES", "SITE_FLUSH_PERIOD", "SITE_STRIP_RECORDS", "LD_CHUNK", "LD_SINK", "LD_SCALE_BITS", "LD_DECAY_MAX_BINS", "LD_DECAY_LOCAL_BINS", "ld_band", "ld_finalize", "site_major"]
