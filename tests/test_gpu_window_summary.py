"""GPU (-m gpu): dst_window_summary / Engine.window_summary — bitwise against dst_summary's definition applied to the
context's own run_windows result of every window (integers equal, sums by their bits): at the window, chunk and tile
edges, on the designed hostile values, across thresholds, past the grid cuts and the 16-bit tallies, with every subset of
NULL arrays, and its state, order and errors."""
import ctypes as C
import itertools

import numpy as np
import pytest

import distance_amd as da
from distance_amd import _lib
from helpers import CODES, KNOWN, random_alignment, uniform_codes
from summary_reference import assert_summary
from tools import synth
from window_summary_cases import ALL, hostile_partner, hostile_set, hostile_windows
from window_summary_reference import assert_window_summary, window_summary

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE, ERR_CAPACITY = 1, 4, 6
MEASURE_ID = {m: k for k, m in enumerate(ALL)}


@pytest.fixture(scope="module")
def eng():
    with da.Engine(0) as e:
        yield e


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype.itemsize == 8 else a


def same(a, b):
    """two window_summary results with identical bytes"""
    return a.keys() == b.keys() and all(bits(a[k]).tobytes() == bits(b[k]).tobytes() for k in a)


def check(eng, measure, windows, threshold, square, what=""):
    """the call against the definition applied to run_windows of the same context; returns (got, want)"""
    n_rows, _ = eng.set_info(0)
    n_cols, _ = eng.set_info(0 if square else 1)
    vals = eng.run_windows(measure, windows, square=square)
    want = window_summary(measure, vals, n_rows, n_cols, square, threshold)
    got = eng.window_summary(measure, windows, threshold, square=square)
    assert_window_summary(got, want, (what, measure, threshold, square))
    return got, want


def edge_windows(length):
    """whole, empty, one site, both cuts in one chunk, cuts at 127 / 128 / 129, a repeat, then all of them in descending order"""
    c = lambda x: min(x, length)
    w = [(0, length), (c(5), c(5)), (length - 1, length), (0, 1), (c(3), c(70)), (0, c(127)), (0, c(128)), (0, c(129)),
         (c(127), length), (c(128), length), (c(129), length), (c(127), c(129)), (c(100), c(257)), (0, length)]
    return np.array(w + w[::-1], np.uint64)


# ---- 1. window edges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [1, 127, 128, 129, 257, 1000])
@pytest.mark.parametrize("n", [2, 3, 9, 65, 257])
def test_window_edges(eng, n, length):
    codes = random_alignment(n, length, seed=1000 * n + length, divergence=0.3)
    nine = random_alignment(9, length, seed=7 + length, divergence=0.3)
    windows = edge_windows(length)
    eng.upload(0, nine)
    eng.upload(1, codes)
    for m in ALL:
        check(eng, m, windows, 0.1 if m not in ("n", "n_high") else 3, False, (n, length))   # the rectangle 9 x n
    eng.upload(0, codes)
    for m in ALL:
        check(eng, m, windows, 0.1 if m not in ("n", "n_high") else 3, True, (n, length))


# ---- 2. tile edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cols", [255, 256, 257, 513])
def test_tile_edges_rectangle(eng, n_cols):
    length = 200
    eng.upload(0, random_alignment(9, length, seed=21, divergence=0.2))
    eng.upload(1, random_alignment(n_cols, length, seed=n_cols, divergence=0.2))
    windows = np.array([(0, length), (120, 140), (199, 200)], np.uint64)
    for m in ALL:
        check(eng, m, windows, 0.15 if m not in ("n", "n_high") else 20, False, n_cols)


def test_tile_edges_square_513(eng):
    # three column tiles add into one row entry, 65 row tiles into one column entry
    length = 200
    eng.upload(0, random_alignment(513, length, seed=513, divergence=0.2))
    windows = np.array([(0, length), (120, 140), (199, 200)], np.uint64)
    for m in ALL:
        check(eng, m, windows, 0.15 if m not in ("n", "n_high") else 20, True)


# ---- 3. hostile values (tests/test_window_summary_host.py holds the set to its design) ----------------------------------------
@pytest.mark.parametrize("square", [True, False])
def test_hostile_values(eng, square):
    eng.upload(0, hostile_set())
    eng.upload(1, hostile_partner())
    windows = hostile_windows()
    for m in ALL:
        got, _ = check(eng, m, windows, 0.5, square)
        if m not in ("n", "n_high"):
            assert got["nan_pairs"][0] > 0 and got["nan_pairs"][11] == got["pairs"][11], m   # (window 11 is empty)
        if m == "jc69":
            assert (got["pairs"] - got["nan_pairs"] - got["summable_pairs"])[0] > 0   # +inf: neither NaN nor summable


# ---- 4. thresholds ---------------------------------------------------------------------------------------------------------------
def test_thresholds(eng):
    eng.upload(0, hostile_set())
    windows = hostile_windows()
    for t in (0, 2, 2.9, np.inf, -1):
        check(eng, "n", windows, t, True)
    assert same(eng.window_summary("n", windows, 2), eng.window_summary("n", windows, 2.9))
    assert not eng.window_summary("n", windows, -1)["links"].any()
    vals = eng.run_windows("raw", windows)
    exact = float(np.sort(vals[0][~np.isnan(vals[0])])[10])   # a pair's own payload: it links, the next larger does not
    for t in (0, exact, float(np.nextafter(exact, 0)), np.inf, -1):
        check(eng, "raw", windows, t, True)
    for m in ("jc69", "k80", "tn93"):
        got, _ = check(eng, m, windows, np.inf, True)
        assert np.array_equal(got["links"], got["pairs"] - got["nan_pairs"])   # +inf links at T = inf
        assert not check(eng, m, windows, -1, True)[0]["within"].any()
    with pytest.raises(da.DistanceError) as e:
        eng.window_summary("raw", windows, float("nan"))
    assert e.value.status == ERR_ARG and "threshold is NaN" in e.value.message


# ---- 5. grid cuts and wide tallies -----------------------------------------------------------------------------------------------
def test_65536_windows_cross_the_grid_cut(eng):
    length = 40
    eng.upload(0, random_alignment(3, length, seed=5, divergence=0.4))
    w = np.arange(65536, dtype=np.uint64)
    begin = w % 41
    end = np.minimum(begin + (w // 41) % 42, length)
    windows = np.stack([begin, end], axis=1)
    distinct, inverse = np.unique(windows, axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    for m in ("n", "raw", "tn93"):
        vals = eng.run_windows(m, windows)
        first = np.array([np.nonzero(inverse == d)[0][0] for d in range(len(distinct))])
        for d, f in enumerate(first):   # (run_windows itself is the same for equal windows)
            assert bits(vals[inverse == d]).tobytes() == bits(vals[f:f + 1]).tobytes() * int((inverse == d).sum())
        ref = window_summary(m, vals[first], 3, 3, True, 0.2 if m != "n" else 5)
        want = {k: v[inverse] for k, v in ref.items()}
        assert_window_summary(eng.window_summary(m, windows, 0.2 if m != "n" else 5), want, m)


def test_tallies_past_16_bits(eng):
    length = 65537
    rng = np.random.default_rng(3)
    known = np.array(KNOWN, np.uint8)
    codes = np.stack([np.full(length, known[0]), np.full(length, known[2]), known[rng.integers(0, 4, length)]])
    eng.upload(0, np.ascontiguousarray(codes))
    windows = np.array([(0, length)], np.uint64)
    for m in ALL:
        got, _ = check(eng, m, windows, 0.5 if m not in ("n", "n_high") else 65536, True)
    assert eng.run_windows("n", windows)[0, 0] == length


# ---- 6. NULL arrays, repeatability ---------------------------------------------------------------------------------------------------
def raw_call(eng, measure, windows, threshold, square, n_rows, want=(True, True, True, True), cap=None, fill=None):
    """the C call with any subset of its four outputs; returns (rc, totals, within, summable, sum) with None for a NULL one"""
    nw = len(windows)
    wb, we = np.ascontiguousarray(windows[:, 0]), np.ascontiguousarray(windows[:, 1])
    tot = (_lib.SummaryTotals * max(nw, 1))()
    entries = nw * n_rows
    within = np.full(max(entries, 1), 0 if fill is None else fill, np.uint32)
    summable = np.full(max(entries, 1), 0 if fill is None else fill, np.uint32)
    sums = np.full(max(entries, 1), 0 if fill is None else fill, np.float64)
    rc = eng._lib.dst_window_summary(eng._h, MEASURE_ID[measure], int(square), 0, 1, wb.ctypes.data, we.ctypes.data, nw,
                                     float(threshold), tot if want[0] else None, within.ctypes.data if want[1] else None,
                                     summable.ctypes.data if want[2] else None, sums.ctypes.data if want[3] else None,
                                     entries if cap is None else cap)
    t = np.frombuffer(bytes(tot), np.uint64).reshape(-1, 5)[:nw]
    return rc, (t if want[0] else None), (within if want[1] else None), (summable if want[2] else None), (sums if want[3] else None)


@pytest.mark.parametrize("square", [True, False])
def test_every_subset_of_null_arrays(eng, square):
    eng.upload(0, hostile_set())
    eng.upload(1, hostile_partner())
    windows = hostile_windows()
    for m in ("n", "raw", "tn93"):
        full = raw_call(eng, m, windows, 0.5, square, 9)
        assert full[0] == 0
        check(eng, m, windows, 0.5, square)
        for want in itertools.product((True, False), repeat=4):
            if not any(want):
                continue
            part = raw_call(eng, m, windows, 0.5, square, 9, want)
            assert part[0] == 0, (m, want)
            for k in range(1, 5):
                if want[k - 1]:
                    assert bits(part[k]).tobytes() == bits(full[k]).tobytes(), (m, want, k)
        # Engine's totals-only form: the same totals
        only = eng.window_summary(m, windows, 0.5, square=square, per_record=False)
        whole = eng.window_summary(m, windows, 0.5, square=square)
        assert "within" not in only and same(only, {k: whole[k] for k in only})


def test_the_same_call_twice_gives_identical_bytes(eng):
    eng.upload(0, random_alignment(300, 700, seed=44, divergence=0.2))
    windows = np.array([(0, 700), (100, 400), (650, 700), (30, 31)], np.uint64)
    for m in ("n", "jc69", "tn93"):
        assert same(eng.window_summary(m, windows, 0.1), eng.window_summary(m, windows, 0.1)), m


# ---- 7. the whole width is dst_summary ---------------------------------------------------------------------------------------------------
def test_whole_width_equals_summary(eng):
    length = 300
    eng.upload(0, random_alignment(65, length, seed=8, divergence=0.3))
    eng.upload(1, random_alignment(40, length, seed=9, divergence=0.3))
    windows = np.array([(0, length)], np.uint64)
    for m in ALL:
        for square in (True, False):
            t = 0.2 if m not in ("n", "n_high") else 60
            got = eng.window_summary(m, windows, t, square=square)
            one = {k: (int(v[0]) if k in ("pairs", "nan_pairs", "summable_pairs", "links") else v[0]) for k, v in got.items()}
            assert_summary(one, eng.summary(m, t, square=square), (m, square))


# ---- 8. state and order ----------------------------------------------------------------------------------------------------------------------
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
    with da.Engine(0) as lazy:
        lazy.set_prep_threshold(0)
        lazy.upload(0, codes)
        assert not lazy.planes_stored(0), "the upload stored every plane: nothing here tests the deferred form"
        lazy.set_path("consensus")
        square_before = {m: lazy.run_square(m, 0, 40) for m in ("n", "tn93")}
        launch, path = lazy.last_launch(), lazy.last_path()
        assert not lazy.planes_stored(0)
        check(lazy, "raw", windows, 0.05, True)
        assert lazy.planes_stored(0)
        assert lazy.last_launch() == launch and lazy.last_path() == path

        def others():
            return (bits(lazy.run_windows("tn93", windows)).tobytes(),
                    tuple(bits(x).tobytes() for x in lazy.nearest_windows("tn93", windows, 3)),
                    tuple(sorted((k, bits(np.asarray(v)).tobytes()) for k, v in lazy.summary("tn93", 0.05).items())))

        before = others()
        launch, path = lazy.last_launch(), lazy.last_path()   # (summary's own slab runs are launches)
        mine = lazy.window_summary("tn93", windows, 0.05)
        assert lazy.last_launch() == launch and lazy.last_path() == path
        assert others() == before
        assert same(lazy.window_summary("tn93", windows, 0.05), mine)
        launch, path = lazy.last_launch(), lazy.last_path()
        check(lazy, "k80", other, 0.05, True)   # a call with a different window table in between
        assert lazy.last_launch() == launch and lazy.last_path() == path
        assert others() == before
        assert same(lazy.window_summary("tn93", windows, 0.05), mine)
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
            eng.window_summary("raw", windows, 0.1, per_record=False)
        return e.value.status, e.value.message

    try:
        for status, message in ThreadRanks(2).run(body):
            assert status == ERR_STATE and "dst_upload_shared runs on the consensus path only" in message
    finally:
        hip.lib.hipFree(d_codes)


# ---- 9. errors ---------------------------------------------------------------------------------------------------------------------------------
def test_errors_in_the_documented_order():
    codes = uniform_codes(9, 200, seed=5)
    windows = np.array([(0, 200), (10, 20), (199, 200)], np.uint64)
    FILL = 0x5A5A5A5A
    lib = da.load()
    with da.Engine(0) as eng:
        h = eng._h

        def call(measure=2, square=1, rs=0, cs=1, wb=windows[:, 0], we=windows[:, 1], nw=3, t=0.1, cap=27, totals=True, rec=True):
            tot = np.full(5 * 3, FILL, np.uint64)
            arrays = [np.full(27, FILL, np.uint32), np.full(27, FILL, np.uint32), np.full(27, FILL, np.uint64)]
            wb = None if wb is None else np.ascontiguousarray(wb)
            we = None if we is None else np.ascontiguousarray(we)
            rc = lib.dst_window_summary(h, measure, square, rs, cs, None if wb is None else wb.ctypes.data,
                                        None if we is None else we.ctypes.data, nw, t, tot.ctypes.data if totals else None,
                                        *[a.ctypes.data if rec else None for a in arrays], cap)
            untouched = bool((tot == FILL).all() and all((a == FILL).all() for a in arrays))
            return rc, untouched, lib.dst_last_error(h).decode(), tot, arrays

        rc, untouched, msg, _, _ = call()
        assert rc == ERR_STATE and msg == "set not uploaded" and untouched
        eng.upload(0, codes)
        rc, untouched, _, tot, arrays = call()
        assert rc == 0 and not untouched
        want = eng.window_summary("raw", windows, 0.1)
        assert np.array_equal(tot.reshape(3, 5)[:, 0], want["pairs"]) and np.array_equal(arrays[0].reshape(3, 9), want["within"])
        nan = float("nan")
        bad = [
            # each line breaks the rule it names and every LATER rule it can: the earlier one speaks
            (dict(nw=da.WINDOWS_MAX + 1, wb=None, measure=9, t=nan), "more than DST_WINDOWS_MAX"),
            (dict(wb=None, measure=9, t=nan), "null pointer"), (dict(we=None), "null pointer"),
            (dict(measure=6, t=nan, totals=False, rec=False), "unknown measure"), (dict(measure=-1), "unknown measure"),
            (dict(t=nan, totals=False, rec=False, square=0, rs=0, cs=0), "threshold is NaN"),
            (dict(totals=False, rec=False, square=0, rs=0, cs=0), "null output pointers"),
            (dict(square=0, rs=0, cs=0, wb=np.array([0, 21, 5], np.uint64)), "row_slot == col_slot"),
            (dict(square=0, rs=0, cs=2), "slot must be 0 or 1"), (dict(square=0, rs=-1, cs=0), "slot must be 0 or 1"),
            (dict(wb=np.array([0, 21, 5], np.uint64), cap=0), "window 1 [21, 20)"),
            (dict(we=np.array([200, 20, 201], np.uint64), cap=0), "window 2 [199, 201)"),
        ]
        for kw, text in bad:
            rc, untouched, msg, _, _ = call(**kw)
            assert rc == ERR_ARG and text in msg and untouched, (kw, rc, msg)
        rc, untouched, msg, _, _ = call(square=0, rs=0, cs=1)
        assert rc == ERR_STATE and msg == "set not uploaded" and untouched
        # capacity: nothing written; without a per-record array rec_cap is not looked at
        rc, untouched, msg, _, _ = call(cap=26)
        assert rc == ERR_CAPACITY and untouched and "rec_cap" in msg
        rc, untouched, _, tot, _ = call(cap=0, rec=False)
        assert rc == 0 and np.array_equal(tot.reshape(3, 5)[:, 3], want["links"])
        # different widths, then the trivial calls: DST_OK, zero counts and sums, pairs set
        eng.upload(1, uniform_codes(4, 100, seed=6))
        rc, untouched, msg, _, _ = call(square=0)
        assert rc == ERR_STATE and untouched
        rc, untouched, _, _, _ = call(nw=0)
        assert rc == 0 and untouched
        # (an upload refuses an empty set, so a square of one record is the call without a pair that can be reached)
        eng.upload(0, codes[:1])
        rc, _, _, tot, arrays = call(cap=3)
        assert rc == 0 and not tot.any() and not arrays[0][:3].any() and (arrays[0][3:] == FILL).all()
        assert not arrays[2][:3].any() and (arrays[2][3:] == FILL).all()
        # per-record arrays of more than 2^31 entries are refused before anything is allocated
        eng.upload(0, uniform_codes(40000, 8, seed=1))
        many = np.zeros(65536, np.uint64)
        rc, untouched, msg, _, _ = call(wb=many, we=many, nw=65536, cap=1 << 40)
        assert rc == ERR_ARG and untouched and "2^31" in msg
