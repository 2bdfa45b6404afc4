"""GPU (-m gpu): dst_window_group_summary / Engine.window_group_summary — bitwise against dst_group_summary's definition
applied to the context's own run_windows result of every window and the labels (integers equal, doubles by their bits): at
the window, chunk and tile edges, at the edges of the by-group reduction (uniform waves, mixed waves, more groups than leader
rounds, more groups than one table batch holds), on the designed hostile values, across thresholds, past the grid cut, the
16-bit tallies and a 64-bit cell sum, with every subset of NULL arrays, and its state, order and errors.  Every check runs
the call twice: with the per-record arrays (the full square) and for the cells alone (the triangle)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import distance_amd as da
from distance_amd import _lib
from group_summary_reference import assert_group_summary, bits
from helpers import CODES, KNOWN, random_alignment, uniform_codes
from tools import synth
from window_group_summary_reference import assert_window_group_summary, check_window_consequences, window_group_summary
from window_summary_cases import ALL, hostile_partner, hostile_set, hostile_windows

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE, ERR_CAPACITY = 1, 4, 6
MEASURE_ID = {m: k for k, m in enumerate(ALL)}
NONE = 0xFFFFFFFF
CELL_KEYS = ("pairs", "nan_pairs", "summable_pairs", "links", "sum", "min", "max")
QUIET_NAN = 0x7FF8000000000000


@pytest.fixture(scope="module")
def eng():
    with da.Engine(0) as e:
        yield e


def same(a, b):
    """two results with identical bytes"""
    return a.keys() == b.keys() and all(bits(a[k]).tobytes() == bits(b[k]).tobytes() for k in a)


def threshold_of(m):
    return 0.15 if m not in ("n", "n_high") else 20


def check(eng, measure, windows, threshold, square, rg, Gr, cg=None, Gc=None, what=""):
    """the call against the definition applied to run_windows of the same context; the cells alone are the same cells;
    returns the result with the per-record tables"""
    n_rows, _ = eng.set_info(0)
    n_cols, _ = eng.set_info(0 if square else 1)
    vals = eng.run_windows(measure, windows, square=square)
    want = window_group_summary(measure, vals, n_rows, n_cols, square, threshold, rg, Gr, cg, Gc)
    kw = dict(threshold=threshold, square=square, col_groups=cg, n_col_groups=Gc)
    got = eng.window_group_summary(measure, windows, rg, Gr, per_record=True, **kw)
    assert_window_group_summary(got, want, (what, measure, threshold, square))
    check_window_consequences(got, rg, square)
    only = eng.window_group_summary(measure, windows, rg, Gr, **kw)
    assert "rec_sum" not in only and same(only, {k: got[k] for k in only}), (what, measure, "the cells alone")
    return got


def edge_windows(length):
    """test_gpu_window_summary's table: whole, empty, one site, both cuts in one chunk, cuts at 127 / 128 / 129, a repeat,
    then all of them in descending order"""
    c = lambda x: min(x, length)
    w = [(0, length), (c(5), c(5)), (length - 1, length), (0, 1), (c(3), c(70)), (0, c(127)), (0, c(128)), (0, c(129)),
         (c(127), length), (c(128), length), (c(129), length), (c(127), c(129)), (c(100), c(257)), (0, length)]
    return np.array(w + w[::-1], np.uint64)


def random_labels(n, G, seed, unassigned=True):
    """labels below G, a third of the records without a group"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, G, n)
    return np.where(rng.random(n) < 1 / 3, -1, g) if unassigned else g


# ---- 1. window, chunk and tile edges ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [1, 127, 128, 129, 257])
@pytest.mark.parametrize("n", [2, 9, 65, 257])
def test_window_edges(eng, n, length):
    codes = random_alignment(n, length, seed=1000 * n + length, divergence=0.3)
    nine = random_alignment(9, length, seed=7 + length, divergence=0.3)
    windows = edge_windows(length)
    rg9, cg = random_labels(9, 2, n), random_labels(n, 3, length)
    eng.upload(0, nine)
    eng.upload(1, codes)
    for m in ALL:
        check(eng, m, windows, 0.1 if m not in ("n", "n_high") else 3, False, rg9, 2, cg, 3, (n, length))   # the rectangle 9 x n
    eng.upload(0, codes)
    for m in ALL:
        check(eng, m, windows, 0.1 if m not in ("n", "n_high") else 3, True, cg, 3, what=(n, length))


@pytest.mark.parametrize("n_cols", [255, 256, 257, 513])
def test_tile_edges_rectangle(eng, n_cols):
    length = 200
    eng.upload(0, random_alignment(9, length, seed=21, divergence=0.2))
    eng.upload(1, random_alignment(n_cols, length, seed=n_cols, divergence=0.2))
    windows = np.array([(0, length), (120, 140), (199, 200)], np.uint64)
    for m in ALL:
        check(eng, m, windows, threshold_of(m), False, random_labels(9, 4, 1), 4, random_labels(n_cols, 5, 2), 5, n_cols)


def test_tile_edges_square_513(eng):
    # three column tiles add into one row's entries, 65 row tiles into one cell
    length = 200
    eng.upload(0, random_alignment(513, length, seed=513, divergence=0.2))
    windows = np.array([(0, length), (120, 140), (199, 200)], np.uint64)
    for m in ALL:
        check(eng, m, windows, threshold_of(m), True, random_labels(513, 3, 3), 3)


# ---- 2. group layouts at the reduction's edges ----------------------------------------------------------------------------------
LAYOUT_N, LAYOUT_LEN = 520, 150
LAYOUT_WINDOWS = np.array([(0, LAYOUT_LEN), (100, 140), (7, 7)], np.uint64)


@pytest.fixture(scope="module")
def layout_sets():
    return (random_alignment(LAYOUT_N, LAYOUT_LEN, seed=77, divergence=0.25), random_alignment(9, LAYOUT_LEN, seed=78, divergence=0.25))


def layouts(n, G):
    """contiguous (equal stretches), interleaved record by record, random with a third of the records unassigned"""
    return {"contiguous": np.arange(n) * G // n, "interleaved": np.arange(n) % G, "random": random_labels(n, G, G)}


@pytest.mark.parametrize("G", [1, 2, 3, 64, 65, 255, 256])
def test_group_counts_and_layouts(eng, layout_sets, G):
    # 32 / 33 column groups is where the table stops holding all eight rows of a tile: 1 .. 3 take one batch, 64 and 65 take
    # batches of four and three rows, 255 and 256 one row each; 64 interleaved groups leave 61 lanes of a wave to single adds
    big, nine = layout_sets
    eng.upload(0, big)
    for name, g in layouts(LAYOUT_N, G).items():
        for m in ("n", "raw", "tn93"):
            check(eng, m, LAYOUT_WINDOWS, threshold_of(m), True, g, G, what=(G, name))
    eng.upload(0, nine)
    eng.upload(1, big)
    Gr = 1 + G % 5   # (another count on the row side)
    for name, g in layouts(LAYOUT_N, G).items():
        check(eng, "k80", LAYOUT_WINDOWS, 0.15, False, np.arange(9) % Gr, Gr, g, G, what=(G, name))


@pytest.mark.parametrize("G", [32, 33])
def test_the_table_batch_threshold(eng, layout_sets, G):
    big, _ = layout_sets
    eng.upload(0, big)
    for name, g in layouts(LAYOUT_N, G).items():
        check(eng, "raw", LAYOUT_WINDOWS, 0.15, True, g, G, what=(G, name))


@pytest.mark.parametrize("cut", [63, 64, 65])
def test_contiguous_groups_cut_inside_a_wave(eng, layout_sets, cut):
    # the first wave of the first column tile is uniform but for its last lane, uniform, and the second wave has one lane of
    # the first group
    big, nine = layout_sets
    g = (np.arange(LAYOUT_N) >= cut).astype(int)
    eng.upload(0, big)
    for m in ("n", "jc69", "tn93"):
        check(eng, m, LAYOUT_WINDOWS, threshold_of(m), True, g, 2, what=cut)
    eng.upload(0, nine)
    eng.upload(1, big)
    check(eng, "raw", LAYOUT_WINDOWS, 0.15, False, np.zeros(9, int), 1, g, 2, what=cut)


def test_a_group_of_one_record_and_tiles_without_groups(eng, layout_sets):
    big, nine = layout_sets
    n = LAYOUT_N
    g = np.arange(n) % 3 + 9
    g[0:8] = np.arange(8)       # a row tile whose eight rows have eight different groups, each of one record
    g[8:16] = -1                # a row tile whose rows have none
    g[256:512] = -1             # a column tile whose columns have none
    eng.upload(0, big)
    for m in ("n", "raw", "tn93"):
        got = check(eng, m, LAYOUT_WINDOWS, threshold_of(m), True, g, 12, what="designed tiles")
        for a in range(8):
            assert not got["pairs"][:, a, a].any() and not got["summable_pairs"][:, a, a].any(), (m, a)
            empty = 0 if m == "n" else QUIET_NAN
            assert (bits(got["min"][:, a, a]) == empty).all() and (bits(got["max"][:, a, a]) == empty).all(), (m, a)
        assert got["rec_summable"][0, 8:16].any()   # a record without a group still has its row
    eng.upload(0, nine)
    eng.upload(1, big)
    rows = np.array([0, 1, 2, 3, 4, 5, 6, 7, -1])   # (the second row tile holds one record, and it has no group)
    check(eng, "raw", LAYOUT_WINDOWS, 0.15, False, rows, 8, g, 12, what="designed tiles, rectangle")
    check(eng, "raw", LAYOUT_WINDOWS, 0.15, False, np.full(9, -1), 3, g, 12, what="no row has a group")   # (a trivial call for the cells)
    check(eng, "raw", LAYOUT_WINDOWS, 0.15, False, rows, 8, np.full(n, -1), 2, what="no column has a group")


# ---- 3. hostile values (tests/test_window_summary_host.py holds the set to its design) ----------------------------------------
HOSTILE_ROWS = np.array([0, 1, 1, 0, 2, -1, 2, 0, 1])
HOSTILE_COLS = np.array([1, 0, -1, 1, 0])


@pytest.mark.parametrize("square", [True, False])
def test_hostile_values(eng, square):
    eng.upload(0, hostile_set())
    eng.upload(1, hostile_partner())
    windows = hostile_windows()
    for m in ALL:
        got = check(eng, m, windows, 0.5, square, HOSTILE_ROWS, 3, HOSTILE_COLS, 2)
        if m not in ("n", "n_high"):
            assert got["nan_pairs"][0].any() and np.array_equal(got["nan_pairs"][11], got["pairs"][11]), m   # (window 11 is empty)
        if m == "jc69":
            assert (got["pairs"] - got["nan_pairs"] - got["summable_pairs"])[0].any()   # +inf: neither NaN nor summable


def test_thresholds(eng):
    eng.upload(0, hostile_set())
    windows = hostile_windows()
    g = HOSTILE_ROWS
    for t in (0, 2, 2.9, np.inf, -1):
        check(eng, "n", windows, t, True, g, 3)
    assert same(eng.window_group_summary("n", windows, g, 3, 2), eng.window_group_summary("n", windows, g, 3, 2.9))
    assert not eng.window_group_summary("n", windows, g, 3, -1)["links"].any()
    vals = eng.run_windows("raw", windows)
    exact = float(np.sort(vals[0][~np.isnan(vals[0])])[10])   # a pair's own payload: it links, the next larger does not
    for t in (0, exact, float(np.nextafter(exact, 0)), np.inf, -1):
        check(eng, "raw", windows, t, True, g, 3)
    for m in ("jc69", "k80", "tn93"):
        got = check(eng, m, windows, np.inf, True, g, 3)
        assert np.array_equal(got["links"], got["pairs"] - got["nan_pairs"])   # +inf links at T = inf
        assert not check(eng, m, windows, -1, True, g, 3)["rec_within"].any()
    with pytest.raises(da.DistanceError) as e:
        eng.window_group_summary("raw", windows, g, 3, float("nan"))
    assert e.value.status == ERR_ARG and "threshold is NaN" in e.value.message


# ---- 4. consequences ---------------------------------------------------------------------------------------------------------------
def test_whole_width_equals_group_summary(eng):
    length = 300
    eng.upload(0, random_alignment(65, length, seed=8, divergence=0.3))
    eng.upload(1, random_alignment(40, length, seed=9, divergence=0.3))
    windows = np.array([(0, length)], np.uint64)
    rg, cg = random_labels(65, 4, 1), random_labels(40, 3, 2)
    for m in ALL:
        for square in (True, False):
            t = 0.2 if m not in ("n", "n_high") else 60
            kw = dict(threshold=t, square=square, col_groups=cg, n_col_groups=3, per_record=True)
            got = eng.window_group_summary(m, windows, rg, 4, **kw)
            assert_group_summary({k: v[0] for k, v in got.items()}, eng.group_summary(m, rg, 4, **kw), (m, square))


def test_one_group_equals_window_summary(eng):
    length = 300
    eng.upload(0, random_alignment(65, length, seed=8, divergence=0.3))
    eng.upload(1, random_alignment(40, length, seed=9, divergence=0.3))
    windows = np.array([(0, length), (100, 230), (127, 129), (9, 9)], np.uint64)
    for m in ALL:
        for square in (True, False):
            t = 0.2 if m not in ("n", "n_high") else 60
            got = eng.window_group_summary(m, windows, np.zeros(65, int), 1, t, square=square, col_groups=np.zeros(40, int),
                                           n_col_groups=1, per_record=True)
            ref = eng.window_summary(m, windows, t, square=square)
            for cell, total in (("pairs", "pairs"), ("nan_pairs", "nan_pairs"), ("summable_pairs", "summable_pairs"),
                                ("links", "links"), ("sum", "total_sum")):
                assert bits(got[cell][:, 0, 0]).tobytes() == bits(ref[total]).tobytes(), (m, square, cell)
            for rec, per in (("rec_within", "within"), ("rec_summable", "summable"), ("rec_sum", "sum")):
                assert bits(got[rec][:, :, 0]).tobytes() == bits(ref[per]).tobytes(), (m, square, rec)


def test_the_same_call_twice_gives_identical_bytes(eng):
    eng.upload(0, random_alignment(300, 700, seed=44, divergence=0.2))
    windows = np.array([(0, 700), (100, 400), (650, 700), (30, 31)], np.uint64)
    g = random_labels(300, 5, 4)
    for m in ("n", "jc69", "tn93"):
        for per_record in (False, True):
            a = eng.window_group_summary(m, windows, g, 5, 0.1, per_record=per_record)
            assert same(a, eng.window_group_summary(m, windows, g, 5, 0.1, per_record=per_record)), (m, per_record)


def raw_call(eng, measure, windows, threshold, square, n_rows, rg, Gr, cg, Gc, want=(True, True, True, True)):
    """the C call with any subset of its four outputs; returns (rc, cells, within, summable, sum) with None for a NULL one"""
    nw = len(windows)
    wb, we = np.ascontiguousarray(windows[:, 0]), np.ascontiguousarray(windows[:, 1])
    rg = np.ascontiguousarray(np.where(np.asarray(rg) < 0, NONE, rg).astype(np.uint32))
    cg = np.ascontiguousarray(np.where(np.asarray(cg) < 0, NONE, cg).astype(np.uint32))
    n_cells, entries = nw * Gr * Gc, nw * n_rows * Gc
    cells = np.zeros(n_cells * 7, np.uint64)
    within, summable, sums = np.zeros(entries, np.uint32), np.zeros(entries, np.uint32), np.zeros(entries, np.float64)
    rc = eng._lib.dst_window_group_summary(eng._h, MEASURE_ID[measure], int(square), 0, 1, wb.ctypes.data, we.ctypes.data, nw,
                                           rg.ctypes.data, Gr, cg.ctypes.data, Gc, float(threshold),
                                           cells.ctypes.data if want[0] else None, n_cells, within.ctypes.data if want[1] else None,
                                           summable.ctypes.data if want[2] else None, sums.ctypes.data if want[3] else None, entries)
    return rc, (cells if want[0] else None), (within if want[1] else None), (summable if want[2] else None), (sums if want[3] else None)


@pytest.mark.parametrize("square", [True, False])
def test_every_subset_of_null_arrays(eng, square):
    eng.upload(0, hostile_set())
    eng.upload(1, hostile_partner())
    windows = hostile_windows()
    rg, Gr = HOSTILE_ROWS, 3
    cg, Gc = (rg, Gr) if square else (HOSTILE_COLS, 2)
    for m in ("n", "raw", "tn93"):
        full = raw_call(eng, m, windows, 0.5, square, 9, rg, Gr, cg, Gc)
        assert full[0] == 0
        checked = check(eng, m, windows, 0.5, square, rg, Gr, cg, Gc)
        assert bits(checked["rec_sum"]).tobytes() == bits(full[4]).tobytes()
        assert np.array_equal(full[1].reshape(-1, 7)[:, 3], checked["links"].reshape(-1))
        for want in itertools.product((True, False), repeat=4):
            if not any(want):
                continue
            part = raw_call(eng, m, windows, 0.5, square, 9, rg, Gr, cg, Gc, want)
            assert part[0] == 0, (m, want)
            for k in range(1, 5):
                if want[k - 1]:
                    assert bits(part[k]).tobytes() == bits(full[k]).tobytes(), (m, want, k)


# ---- 5. boundaries -------------------------------------------------------------------------------------------------------------------
def test_65536_windows_cross_the_grid_cut(eng):
    length = 40
    eng.upload(0, random_alignment(3, length, seed=5, divergence=0.4))
    w = np.arange(65536, dtype=np.uint64)
    begin = w % 41
    end = np.minimum(begin + (w // 41) % 42, length)
    windows = np.stack([begin, end], axis=1)
    distinct, inverse = np.unique(windows, axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    first = np.array([np.nonzero(inverse == d)[0][0] for d in range(len(distinct))])
    g = np.array([0, 1, 0])
    for m in ("n", "raw", "tn93"):
        vals = eng.run_windows(m, windows)
        assert bits(vals).tobytes() == bits(vals[first][inverse]).tobytes()   # (run_windows itself is the same for equal windows)
        t = 0.2 if m != "n" else 5
        ref = window_group_summary(m, vals[first], 3, 3, True, t, g, 2)
        want = {k: v[inverse] for k, v in ref.items()}
        assert_window_group_summary(eng.window_group_summary(m, windows, g, 2, t, per_record=True), want, m)
        assert_window_group_summary(eng.window_group_summary(m, windows, g, 2, t), want, m)


def test_tallies_past_16_bits(eng):
    length = 65537
    rng = np.random.default_rng(3)
    known = np.array(KNOWN, np.uint8)
    codes = np.stack([np.full(length, known[0]), np.full(length, known[2]), known[rng.integers(0, 4, length)]])
    eng.upload(0, np.ascontiguousarray(codes))
    windows = np.array([(0, length)], np.uint64)
    for m in ALL:
        check(eng, m, windows, 0.5 if m not in ("n", "n_high") else 65536, True, np.array([1, 0, 1]), 2)
    assert eng.run_windows("n", windows)[0, 0] == length


def test_a_cell_sum_past_64_bits_has_its_closed_form(eng):
    # 12,000 records all A and 12,000 all C: raw is 0.0 inside a half and 1.0 across, in both windows.  The 1.44e8 pairs
    # across the halves sum to 1.44e8 x 2^37 fixed-point units, more than 2^64: the carry into the high word is needed.
    half = 12_000
    known = np.array(KNOWN, np.uint8)
    codes = np.ascontiguousarray(np.repeat(np.array([[known[0]] * 8, [known[1]] * 8], np.uint8), half, axis=0))
    eng.upload(0, codes)
    windows = np.array([(0, 8), (0, 4)], np.uint64)
    inside, across, both = half * (half - 1) // 2, half * half, 2 * half * (2 * half - 1) // 2
    assert across * 2 ** 37 > 2 ** 64
    two = eng.window_group_summary("raw", windows, np.repeat([0, 1], half), 2, 0.5)
    for w in range(2):
        assert two["pairs"][w].tolist() == [[inside, across], [across, inside]]
        assert two["summable_pairs"][w].tolist() == [[inside, across], [across, inside]] and not two["nan_pairs"][w].any()
        assert two["links"][w].tolist() == [[inside, 0], [0, inside]]
        assert two["sum"][w].tolist() == [[0.0, 144000000.0], [144000000.0, 0.0]]
        assert two["min"][w].tolist() == [[0.0, 1.0], [1.0, 0.0]] and two["max"][w].tolist() == [[0.0, 1.0], [1.0, 0.0]]
    one = eng.window_group_summary("raw", windows, np.zeros(2 * half, int), 1, 0.5)
    for w in range(2):
        assert one["pairs"][w, 0, 0] == both and one["summable_pairs"][w, 0, 0] == both and one["nan_pairs"][w, 0, 0] == 0
        assert one["links"][w, 0, 0] == 2 * inside and one["sum"][w, 0, 0] == 144000000.0
        assert one["min"][w, 0, 0] == 0.0 and one["max"][w, 0, 0] == 1.0


# ---- 6. state and order ----------------------------------------------------------------------------------------------------------------
def test_deferred_planes_untouched_state_and_order():
    n, length = 1100, 3333
    rng = np.random.default_rng(31)
    codes = synth.alignment(synth.SEED ^ 31, n, length)
    for r in rng.choice(n, 50, replace=False):
        at = rng.choice(length, 20, replace=False)
        codes[r, at] = CODES[rng.integers(0, 17, len(at))]
    codes = np.ascontiguousarray(codes[:300])
    windows = np.array([(0, length), (100, 1100), (127, 129), (3332, 3333), (500, 500)], np.uint64)
    other = np.array([(5, 3000), (0, 10)], np.uint64)
    g, other_g = random_labels(300, 4, 1), random_labels(300, 40, 2)
    with da.Engine(0) as lazy:
        lazy.set_prep_threshold(0)
        lazy.upload(0, codes)
        assert not lazy.planes_stored(0), "the upload stored every plane: nothing here tests the deferred form"
        lazy.set_path("consensus")
        square_before = {m: lazy.run_square(m, 0, 40) for m in ("n", "tn93")}
        launch, path = lazy.last_launch(), lazy.last_path()
        assert not lazy.planes_stored(0)
        check(lazy, "raw", windows, 0.05, True, g, 4)
        assert lazy.planes_stored(0)
        assert lazy.last_launch() == launch and lazy.last_path() == path

        def flat(d):
            return tuple(sorted((k, bits(np.asarray(v)).tobytes()) for k, v in d.items()))

        def others():
            return (bits(lazy.run_windows("tn93", windows)).tobytes(),
                    tuple(bits(x).tobytes() for x in lazy.nearest_windows("tn93", windows, 3)),
                    flat(lazy.window_summary("tn93", windows, 0.05)), flat(lazy.group_summary("tn93", g, 4, 0.05, per_record=True)),
                    flat(lazy.summary("tn93", 0.05)))

        before = others()
        launch, path = lazy.last_launch(), lazy.last_path()   # (summary's own slab runs are launches)
        mine = lazy.window_group_summary("tn93", windows, g, 4, 0.05, per_record=True)
        cells = lazy.window_group_summary("tn93", windows, g, 4, 0.05)
        assert lazy.last_launch() == launch and lazy.last_path() == path
        assert others() == before
        assert same(lazy.window_group_summary("tn93", windows, g, 4, 0.05, per_record=True), mine)
        launch, path = lazy.last_launch(), lazy.last_path()
        check(lazy, "k80", other, 0.05, True, other_g, 40)   # a call with another window table and other labels in between
        assert lazy.last_launch() == launch and lazy.last_path() == path
        assert others() == before
        assert same(lazy.window_group_summary("tn93", windows, g, 4, 0.05, per_record=True), mine)
        assert same(lazy.window_group_summary("tn93", windows, g, 4, 0.05), cells)
        for m, v in square_before.items():
            assert lazy.run_square(m, 0, 40).tobytes() == v.tobytes() and lazy.last_path() == "consensus", m


class Hip:
    """device memory without torch"""

    def __init__(self):
        self.lib = C.CDLL("libamdhip64.so")
        self.lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.lib.hipFree.argtypes = [C.c_void_p]
        self.lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def to_device(self, a):
        p = C.c_void_p()
        assert self.lib.hipMalloc(C.byref(p), a.nbytes) == 0
        assert self.lib.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
        return p.value


def test_shared_set_is_refused():
    from shared_ranks import ThreadRanks
    n, length = 2_500, 3_000   # (a shape of test_gpu_shared: the lists fit their blocks, no rank falls back to a full upload)
    codes = synth.alignment(synth.SEED ^ 9, n, length)
    hip = Hip()
    d_codes = hip.to_device(codes)
    windows = np.array([(0, 100)], np.uint64)

    def body(rank, eng, comm):
        eng.upload_shared(comm, 0, d_codes, n, length, length, with_counts=True)
        assert eng.shared_stats()["fallbacks"] == 0
        with pytest.raises(da.DistanceError) as e:
            eng.window_group_summary("raw", windows, np.zeros(n, int), 1, 0.1)
        return e.value.status, e.value.message

    try:
        for status, message in ThreadRanks(2).run(body):
            assert status == ERR_STATE and "dst_upload_shared runs on the consensus path only" in message
    finally:
        hip.lib.hipFree(d_codes)


# ---- 7. errors ---------------------------------------------------------------------------------------------------------------------------
def test_errors_in_the_documented_order():
    codes = uniform_codes(9, 200, seed=5)
    windows = np.array([(0, 200), (10, 20), (199, 200)], np.uint64)
    labels = np.array([0, 1, 0, 1, NONE, 1, 0, 0, 1], np.uint32)
    FILL = 0x5A5A5A5A
    CELLS, REC = 3 * 2 * 2, 3 * 9 * 2
    lib = da.load()
    with da.Engine(0) as eng:
        h = eng._h

        def call(measure=2, square=1, rs=0, cs=1, wb=windows[:, 0], we=windows[:, 1], nw=3, rg=labels, Gr=2, cg=labels, Gc=2, t=0.1,
                 cells_cap=CELLS, rec_cap=REC, cells=True, rec=True):
            out = np.full(7 * CELLS, FILL, np.uint64)
            arrays = [np.full(REC, FILL, np.uint32), np.full(REC, FILL, np.uint32), np.full(REC, FILL, np.uint64)]
            keep = [None if x is None else np.ascontiguousarray(x) for x in (wb, we, rg, cg)]
            ptr = [None if x is None else x.ctypes.data for x in keep]
            rc = lib.dst_window_group_summary(h, measure, square, rs, cs, ptr[0], ptr[1], nw, ptr[2], Gr, ptr[3], Gc, t,
                                              out.ctypes.data if cells else None, cells_cap,
                                              *[a.ctypes.data if rec else None for a in arrays], rec_cap)
            untouched = bool((out == FILL).all() and all((a == FILL).all() for a in arrays))
            return rc, untouched, lib.dst_last_error(h).decode(), out, arrays

        rc, untouched, msg, _, _ = call()
        assert rc == ERR_STATE and msg == "set not uploaded" and untouched
        eng.upload(0, codes)
        rc, untouched, _, out, arrays = call()
        assert rc == 0 and not untouched
        want = eng.window_group_summary("raw", windows, labels.astype(np.int64), 2, 0.1, per_record=True)
        assert np.array_equal(out.reshape(3, 2, 2, 7)[..., 0], want["pairs"]) and np.array_equal(out.reshape(3, 2, 2, 7)[..., 3], want["links"])
        assert np.array_equal(arrays[0].reshape(3, 9, 2), want["rec_within"])
        # the square ignores col_group and n_col_groups
        rc, _, _, again, _ = call(cg=None, Gc=0)
        assert rc == 0 and again.tobytes() == out.tobytes()
        nan = float("nan")
        wrong = labels.copy()
        wrong[4] = 7
        bad_window = np.array([0, 21, 5], np.uint64)
        bad = [
            # each line breaks the rule it names and every LATER rule it can: the earlier one speaks
            (dict(nw=da.WINDOWS_MAX + 1, wb=None, measure=9, t=nan), "more than DST_WINDOWS_MAX"),
            (dict(wb=None, measure=9, t=nan), "null pointer"), (dict(we=None), "null pointer"),
            (dict(measure=6, t=nan, cells=False, rec=False, rg=None), "unknown measure"), (dict(measure=-1), "unknown measure"),
            (dict(t=nan, cells=False, rec=False, rg=None, Gr=0, square=0, rs=0, cs=0), "threshold is NaN"),
            (dict(cells=False, rec=False, rg=None, Gr=0, square=0, rs=0, cs=0), "null cells pointer and no per-record array"),
            (dict(rg=None, Gr=0, square=0, rs=0, cs=0), "null row_group pointer"),
            (dict(cg=None, Gc=0, square=0, rs=0, cs=0), "null col_group pointer"),
            (dict(Gr=0, square=0, rs=0, cs=0, wb=bad_window), "a group count must be between 1 and 256"),
            (dict(Gr=257, wb=bad_window), "a group count must be between 1 and 256"),
            (dict(Gc=257, square=0, rs=0, cs=0), "a group count must be between 1 and 256"),
            (dict(Gc=0, square=0, rs=0, cs=0), "a group count must be between 1 and 256"),
            (dict(square=0, rs=0, cs=0, wb=bad_window, rg=wrong), "row_slot == col_slot"),
            (dict(square=0, rs=0, cs=2), "slot must be 0 or 1"), (dict(square=0, rs=-1, cs=0), "slot must be 0 or 1"),
            (dict(wb=bad_window, rg=wrong, cells_cap=0, rec_cap=0), "window 1 [21, 20)"),
            (dict(we=np.array([200, 20, 201], np.uint64), cells_cap=0), "window 2 [199, 201)"),
            (dict(rg=wrong, cells_cap=0, rec_cap=0),
             "group summary: set record 4 has label 7, which is neither below the group count 2 nor DST_GROUP_NONE"),
        ]
        for kw, text in bad:
            rc, untouched, msg, _, _ = call(**kw)
            assert rc == ERR_ARG and text in msg and untouched, (kw, rc, msg)
        rc, untouched, msg, _, _ = call(square=0, rs=0, cs=1)
        assert rc == ERR_STATE and msg == "set not uploaded" and untouched
        # capacity: nothing written; each cap is looked at only when its array is given
        rc, untouched, msg, _, _ = call(cells_cap=CELLS - 1)
        assert rc == ERR_CAPACITY and untouched and "cells_cap" in msg
        rc, untouched, msg, _, _ = call(rec_cap=REC - 1)
        assert rc == ERR_CAPACITY and untouched and "rec_cap" in msg
        rc, _, _, only, _ = call(rec_cap=0, rec=False)
        assert rc == 0 and only.tobytes() == out.tobytes()
        rc, _, _, _, only = call(cells_cap=0, cells=False)
        assert rc == 0 and all(a.tobytes() == b.tobytes() for a, b in zip(only, arrays))
        # the rectangle: the column side's labels are checked after the row side's, and named
        eng.upload(1, codes[:4])
        rc, untouched, msg, _, _ = call(square=0, cg=np.array([0, 1, 5, 9], np.uint32), cells_cap=0)
        assert rc == ERR_ARG and untouched and "group summary: column record 2 has label 5" in msg
        rc, untouched, msg, _, _ = call(square=0, rg=wrong, cg=np.array([0, 1, 5, 9], np.uint32))
        assert rc == ERR_ARG and untouched and "group summary: row record 4 has label 7" in msg
        # different widths, then the trivial calls: DST_OK, zero counts and sums, pairs from the group sizes, empty min / max
        eng.upload(1, uniform_codes(4, 100, seed=6))
        rc, untouched, msg, _, _ = call(square=0, cg=labels[:4])
        assert rc == ERR_STATE and untouched
        rc, untouched, _, _, _ = call(nw=0)
        assert rc == 0 and untouched

        def is_empty(out, arrays, pairs, nw=3):
            c = out.reshape(3, 2, 2, 7)[:nw]
            return bool(np.array_equal(c[..., 0], np.broadcast_to(np.array(pairs, np.uint64), (nw, 2, 2))) and
                        not c[..., 1:5].any() and (c[..., 5:] == QUIET_NAN).all() and not any(a.any() for a in arrays))

        none = np.full(9, NONE, np.uint32)
        rc, _, _, out, arrays = call(rg=none)   # no record of the set is assigned
        assert rc == 0 and is_empty(out, arrays, [[0, 0], [0, 0]])
        eng.upload(1, codes[:4])
        rc, _, _, out, arrays = call(square=0, cg=none[:4])   # no record of the column side is assigned
        assert rc == 0 and is_empty(out, arrays, [[0, 0], [0, 0]])
        rc, _, _, out, _ = call(square=0, rg=none, cg=labels[:4], rec=False)   # the cells alone while no row record is assigned
        assert rc == 0 and is_empty(out, [], [[0, 0], [0, 0]])
        # (an upload refuses an empty set, so a square of one record is the call without a pair that can be reached)
        eng.upload(0, codes[:1])
        rc, _, _, out, arrays = call(rg=labels[:1], cells_cap=CELLS, rec_cap=6)
        assert rc == 0 and is_empty(out, [a[:6] for a in arrays], [[0, 0], [0, 0]]) and all((a[6:] == FILL).all() for a in arrays)
        # more than 2^31 cells or per-record entries are refused before anything is allocated
        eng.upload(0, uniform_codes(300, 8, seed=1))
        many = np.zeros(65536, np.uint64)
        g = (np.arange(300) % 256).astype(np.uint32)
        rc, untouched, msg, _, _ = call(wb=many, we=many, nw=65536, rg=g, Gr=256, cells_cap=1 << 40, rec_cap=1 << 40)
        assert rc == ERR_ARG and untouched and "2^31 cells" in msg
        rc, untouched, msg, _, _ = call(wb=many, we=many, nw=65536, rg=g, Gr=256, cells_cap=1 << 40, rec_cap=1 << 40, rec=False)
        assert rc == ERR_ARG and untouched and "2^31 cells" in msg
        g = (np.arange(300) % 128).astype(np.uint32)   # 2^30 cells, 300 x 2^23 entries
        rc, untouched, msg, _, _ = call(wb=many, we=many, nw=65536, rg=g, Gr=128, cells_cap=1 << 40, rec_cap=1 << 40, cells=False)
        assert rc == ERR_ARG and untouched and "per-record arrays of more than 2^31 entries" in msg
