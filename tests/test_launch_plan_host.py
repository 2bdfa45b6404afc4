"""CPU: dst_plan_consensus_launch — which consensus pair kernel variant and tile height a launch gets — against a
restatement of its three rules, swept over both sides of every threshold; and the census of
test_gpu_launch_variants.py (its table of instantiations, its cases' shapes) against the plan, so that what the GPU
module relies on is checked without a GPU."""
import itertools

import pytest

import distance_amd as da
import test_gpu_launch_variants as census

ALL = ("n", "n_high", "raw", "jc69", "k80", "tn93")
KINDS = (da.OUT_DISTANCE, da.OUT_TALLY, da.OUT_TALLY16)
PANEL = 2048


def restated(measure, kind, wide, square, n_rows, n_cols, pairs, events, lst, run_adds, hot):
    """(EW, heavy_events, rows per tile, tiles) by the three rules of DESIGN.md 3c'"""
    # 1. rows per tile: 32, halved down to 8 while the launch has fewer than 8 x 768 tiles
    panels = -(-n_cols // PANEL)
    tiles = lambda r: panels * -(-n_rows // r) // (2 if square else 1)                    # noqa: E731
    rows = 32
    while rows > 8 and tiles(rows) < 8 * 768:
        rows //= 2
    # 2. heavy_events: 2 above one event per pair, 1 above 0.3 or lists beyond 100 entries or when the 4 + 4 split helps
    split_helps = measure in ("n", "n_high", "raw", "k80") and (run_adds > 0 or hot or pairs < 120_000_000)
    load = events + run_adds
    heavy = 2 if load > 1.0 else 1 if load > 0.3 or lst > 100.0 or split_helps else 0
    # 3. EW: 8 (no roles), 4, or the output's default: 2; tn93's distance 8, wide 1
    tn93_out = measure == "tn93" and kind == da.OUT_DISTANCE
    ew = 8 if heavy == 2 else 4 if heavy == 1 else ((1 if wide else 8) if tn93_out else 2)
    return ew, heavy, rows, tiles(rows)


def planned(measure, kind, wide, square, n_rows, n_cols, pairs, events, lst, run_adds, hot):
    d = da.plan_consensus_launch(measure, kind, wide, square, n_rows, n_cols, pairs, events, lst, run_adds, hot)
    assert d["measure"] == measure and d["out_kind"] == kind and d["wide"] == wide and d["square"] == square
    assert d["family"] == census.FAMILY[measure] and d["hot"] == hot and d["run_records"] == (run_adds > 0)
    assert d["path"] == ("hybrid" if hot else "consensus") and d["pairs"] == pairs and d["tile_cols"] == PANEL
    return d


# record counts that give each tile height (square: n x n, rectangle: n rows against 1.5 n columns), on either side of
# 1.2e8 pairs: 15,492 is the last square below it
SHAPES = [(True, 300), (True, 15492), (True, 15493), (True, 16000), (True, 22000), (True, 30000), (True, 50000),
          (False, 64), (False, 9000), (False, 16384), (False, 3000)]


def shape_of(square, n):
    cols = n if square else n * 3 // 2
    return n, cols, n * (n - 1) // 2 if square else n * cols


def test_plan_follows_the_three_rules_on_both_sides_of_every_threshold():
    heights, splits = set(), set()
    checked = 0
    for (square, n), measure, kind, wide in itertools.product(SHAPES, ALL, KINDS, (False, True)):
        if wide and kind == da.OUT_TALLY16:
            continue
        n_rows, n_cols, pairs = shape_of(square, n)
        for events, lst, run_adds, hot in itertools.product((0.0, 0.1, 0.29, 0.3, 0.31, 0.99, 1.0, 1.01, 7.0),
                                                            (5.0, 99.0, 100.0, 100.5, 2000.0), (0.0, 0.02, 0.5), (False, True)):
            d = planned(measure, kind, wide, square, n_rows, n_cols, pairs, events, lst, run_adds, hot)
            want = restated(measure, kind, wide, square, n_rows, n_cols, pairs, events, lst, run_adds, hot)
            assert (d["event_waves"], d["heavy_events"], d["rows_per_tile"], d["tiles"]) == want, \
                (measure, kind, wide, square, n, events, lst, run_adds, hot, d)
            heights.add(d["rows_per_tile"])
            splits.add(d["event_waves"])
            checked += 1
    assert heights == {8, 16, 32} and splits == {1, 2, 4, 8} and checked > 50_000


def test_pair_count_threshold_is_at_120_million_pairs():
    for measure in ("n", "n_high", "raw", "k80"):
        below = da.plan_consensus_launch(measure, 0, False, True, 16000, 16000, 119_999_999, 0.1, 15.0)
        at = da.plan_consensus_launch(measure, 0, False, True, 16000, 16000, 120_000_000, 0.1, 15.0)
        assert (below["event_waves"], at["event_waves"]) == (4, 2), measure
    for measure, ew in (("jc69", 2), ("tn93", 8)):        # never by size: jc69 wants its six output waves, tn93 has no roles
        assert da.plan_consensus_launch(measure, 0, False, True, 300, 300, 44850, 0.1, 15.0)["event_waves"] == ew


def test_bad_arguments_are_refused():
    lib = da.load()
    import ctypes as C
    from distance_amd._lib import LaunchInfo
    li = LaunchInfo()
    ok = (2, 0, 0, 1, 100, 100, 4950, 0.1, 10.0, 0.0, 0)
    assert lib.dst_plan_consensus_launch(*ok, C.byref(li)) == 0
    assert lib.dst_plan_consensus_launch(*ok, None) == 1
    for at, bad in ((0, 6), (0, -1), (1, 3), (7, -0.5), (7, float("nan")), (8, -1.0), (9, float("nan"))):
        args = list(ok)
        args[at] = bad
        assert lib.dst_plan_consensus_launch(*args, C.byref(li)) == 1, (at, bad)
    assert lib.dst_plan_consensus_launch(2, da.OUT_TALLY16, 1, 1, 100, 100, 4950, 0.1, 10.0, 0.0, 0, C.byref(li)) == 1
    assert lib.dst_last_launch(None, C.byref(li)) == 1


def test_the_census_table_is_what_the_plan_can_return():
    """every (family, wide, out, EW) the plan function gives for any measure, output, width and load is in the GPU module's
    table, and every entry of the table is given for some input"""
    reached = set()
    for measure, kind, wide in itertools.product(ALL, KINDS, (False, True)):
        if wide and kind == da.OUT_TALLY16:
            continue
        for events, pairs in itertools.product((0.1, 0.5, 3.0), (1000, 500_000_000)):
            d = da.plan_consensus_launch(measure, kind, wide, True, 32000, 32000, pairs, events, 15.0)
            reached.add((d["family"], d["wide"], census.out_name(measure, kind), d["event_waves"]))
    assert reached == census.TABLE and len(census.TABLE) == 65


@pytest.mark.parametrize("name", sorted(census.CASES))
def test_the_census_cases_reach_the_variant_they_name(name):
    """each case of the GPU module, with the statistics its generator is expected to give (and at 0.7 and 1.4 times
    them: the margin the shapes keep from the thresholds), gets the wave split and tile height it asserts on the GPU"""
    c = census.CASES[name]
    square, n_rows, n_cols, pairs = census.case_shape(c)
    wide = c["L"] >= 65536
    for (measure, kind), scale in itertools.product(c["runs"], (0.7, 1.0, 1.4)):
        d = da.plan_consensus_launch(measure, kind, wide, square, n_rows, n_cols, pairs, c["events"] * scale, c["list"] * scale,
                                     c.get("run_adds", 0.0), c["path"] == "hybrid")
        got = (d["family"], d["wide"], census.out_name(measure, kind), d["event_waves"])
        assert got == census.expected_of(c, measure, kind) and d["rows_per_tile"] == c["rows"], (name, measure, kind, scale, d)
        assert got in census.TABLE


def test_the_census_cases_cover_the_table():
    """the cases' launches name every instantiation of the table, and the default split at each tile height for every
    family's native output: what the closing test of the GPU module then sees in the reports"""
    named, heights = set(), {}
    for c in census.CASES.values():
        for measure, kind in c["runs"]:
            key = census.expected_of(c, measure, kind)
            named.add(key)
            heights.setdefault(key, set()).add(c["rows"])
    assert named == census.TABLE
    for measure in ALL:
        out = census.NATIVE[measure]
        assert heights[(census.FAMILY[measure], False, out, census.default_ew(out, False))] >= {8, 16, 32}, measure


def test_the_five_large_shapes():
    """the pair counts, panels and tile heights DESIGN.md 3c' tabulates for the default-split cases"""
    for name, pairs, panels, rows in (("square_16000", 127_992_000, 8, 8), ("square_22000", 241_989_000, 11, 16),
                                      ("square_30000", 449_985_000, 15, 32), ("wide_16000", 127_992_000, 8, 8),
                                      ("rect_16384_x_24576", 402_653_184, 12, 32)):
        c = census.CASES[name]
        square, n_rows, n_cols, p = census.case_shape(c)
        assert p == pairs and -(-n_cols // PANEL) == panels and c["rows"] == rows and c["heavy"] == 0
        assert pairs >= 120_000_000
