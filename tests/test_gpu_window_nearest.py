"""GPU (-m gpu): dst_nearest_windows / Engine.nearest_windows, the k nearest records of every (row record, window) — exact
against the oracle on the cut columns and against the context's own run_windows, across slabs, with ties and special values,
at the column and list edges, and its errors."""
import ctypes as C

import numpy as np
import pytest

import distance_amd as da
from helpers import CODES, random_alignment, uniform_codes
from test_gpu_nearest import datasets
from tools import synth
from window_nearest_reference import full_rect, full_square, nearest, oracle_payloads, take
from window_reference import ALL, WIDTH, expected_tallies

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE, ERR_CAPACITY = 1, 4, 6
A, G, Cc, T, N = 136, 72, 40, 24, 240


@pytest.fixture(scope="module")
def eng():
    with da.Engine(0) as e:
        yield e


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype.itemsize == 8 else a


def same_bits(got, want):
    """equal bits, or both NaN (the oracle's NaN and the device's may differ in sign)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype.kind != "f":
        return got.dtype == want.dtype and np.array_equal(got, want)
    return got.shape == want.shape and bool(((got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))).all())


def from_run_windows(eng, measure, windows, square):
    """(payloads, tallies) of every (window, row record, column record) from the engine's own full window runs"""
    n_rows, _ = eng.set_info(0)
    n_cols, _ = eng.set_info(0 if square else 1)
    vals = eng.run_windows(measure, windows, square=square)
    tal = eng.run_windows(measure, windows, square=square, tallies=True)
    if square:
        return full_square(vals, n_rows), full_square(tal, n_rows)
    return full_rect(vals, n_rows, n_cols), full_rect(tal, n_rows, n_cols)


def check(eng, measure, windows, k, square, payloads, tallies, rb=0, re=None, max_entries=0):
    """the call's three outputs against full payloads / tallies [n_windows, rows of the set, n_cols]"""
    re = payloads.shape[1] if re is None else re
    idx, vals, tal = eng.nearest_windows(measure, windows, k, square=square, row_begin=rb, row_end=re, tallies=True,
                                         max_entries=max_entries)
    want = nearest(payloads[:, rb:re], k, square=square, row_begin=rb)
    what = (measure, k, square, rb, re, max_entries)
    assert idx.dtype == np.uint32 and idx.shape == want.shape, what
    assert np.array_equal(idx, want), what
    assert same_bits(vals, take(payloads, idx, rb)), what
    assert tal.shape == idx.shape + (WIDTH[measure],) and np.array_equal(tal, take(tallies, idx, rb)), what
    return idx, vals, tal


# ---- 1. the rectangle, exact against the oracle --------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", ["n", "n_high", "raw"])
def test_rectangle_exact_against_oracle(eng, measure):
    rows = random_alignment(11, 700, seed=51, p_ambig=0.05, p_gap=0.05, divergence=0.2)
    cols = random_alignment(300, 700, seed=52, p_ambig=0.05, p_gap=0.05, divergence=0.2, root=rows[0])
    windows = np.array([(0, 700), (0, 1), (127, 129), (128, 256), (5, 5), (300, 700), (127, 129), (200, 400)], np.uint64)
    payloads = oracle_payloads(measure, rows, cols, windows)
    tallies = full_rect(expected_tallies(measure, rows, cols, windows), 11, 300)
    eng.set_path("auto")
    eng.upload(0, rows)
    eng.upload(1, cols)
    for k in (1, 5, 64, 65, 256):
        idx, _, _ = check(eng, measure, windows, k, False, payloads, tallies)
        assert idx.shape == (11, 8, k)
    check(eng, measure, windows, 7, False, payloads, tallies, rb=3, re=9)


# ---- 2. the square --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [255, 256, 257, 270])
def test_square_sizes_and_row_ranges(eng, n):
    length = 300
    codes = random_alignment(n, length, seed=60 + n, p_ambig=0.05, p_gap=0.05, divergence=0.2)
    # the base composition differs between the two halves: tn93's per-window counts are not the whole width's
    codes[:, :150][codes[:, :150] == G] = A
    codes[::3, 150:][codes[::3, 150:] == A] = Cc
    windows = np.array([(0, 300), (0, 150), (150, 300), (140, 160)], np.uint64)
    eng.set_path("auto")
    eng.upload(0, codes)
    for measure in ("n", "raw"):
        payloads = oracle_payloads(measure, codes, None, windows, square=True)
        tallies = full_square(expected_tallies(measure, codes, None, windows, square=True), n)
        for rb, re in ((0, n), (250, min(260, n)), (0, 1)):
            k = 254 if rb else 6   # (254 of the 254 .. 269 candidates: records before and behind i among them)
            idx, _, _ = check(eng, measure, windows, k, True, payloads, tallies, rb, re)
            rows = np.arange(rb, re)[:, None, None]
            assert not (idx == rows).any()
            if rb:
                assert (idx < rows).any() and (idx > rows).any()   # neighbours on both sides of i
    payloads, tallies = from_run_windows(eng, "tn93", windows, True)
    counts = eng.window_base_counts(0, windows)
    assert not np.array_equal(counts[1], counts[2])
    for rb, re in ((0, n), (250, min(260, n)), (0, 1)):
        idx, vals, tal = check(eng, "tn93", windows, 6, True, payloads, tallies, rb, re)
    # the value is the canonical pair's: the host's finalisation with the counts in that order, within the device's 1e-12
    i = n - 1
    idx, vals, tal = eng.nearest_windows("tn93", windows, 6, row_begin=i, row_end=n, tallies=True)
    for w in range(len(windows)):
        for e in range(6):
            j = int(idx[-1, w, e])
            assert j < i
            f = da.finalize("tn93", tal[-1, w, e], counts[w, j], counts[w, i])
            v = float(vals[-1, w, e])
            assert (f != f and v != v) or f == v or abs(f - v) <= 1e-12, (n, w, e, f, v)


# ---- 3. every measure on dense, consensus and hybrid uploads -----------------------------------------------------------------
@pytest.fixture(scope="module")
def sets():
    return datasets()


@pytest.mark.parametrize("path", ["dense", "consensus", "hybrid"])
@pytest.mark.parametrize("kind", ["low", "clade", "nrun", "uniform"])
def test_every_measure_every_upload(sets, path, kind):
    codes = sets[kind]
    n, length = codes.shape
    windows = np.array([(0, length), (0, length // 3), (length // 3, min(length // 3 + 130, length)), (7, 7), (length - 40, length)], np.uint64)
    with da.Engine(0) as e:
        e.set_prep_threshold(0)
        e.set_path(path)
        e.upload(0, codes)
        for m in ALL:
            payloads, tallies = from_run_windows(e, m, windows, True)
            check(e, m, windows, 9, True, payloads, tallies)


# ---- 4. ties and special values -------------------------------------------------------------------------------------------------
def test_identical_records_in_index_order(eng):
    codes = np.tile(random_alignment(1, 200, seed=71), (70, 1))
    windows = np.array([(0, 200), (50, 50), (3, 140)], np.uint64)
    eng.set_path("auto")
    eng.upload(0, codes)
    for m in ("n_high", "raw", "tn93"):
        idx, vals = eng.nearest_windows(m, windows, 12)
        for i in range(70):
            want = [j for j in range(70) if j != i][:12]
            assert all(list(idx[i, w]) == want for w in range(3)), (m, i)
        assert (vals[:, 0] == 0).all() and (vals[:, 2] == 0).all()
        assert np.isnan(vals[:, 1]).all() if m == "raw" else True


def test_blocks_of_duplicates(eng):
    base = random_alignment(5, 400, seed=72, divergence=0.3)
    codes = np.ascontiguousarray(base[np.arange(60) % 5])
    windows = np.array([(0, 400), (100, 230), (399, 400)], np.uint64)
    eng.set_path("auto")
    eng.upload(0, codes)
    for m in ("n_high", "raw", "k80", "tn93"):
        payloads, tallies = from_run_windows(eng, m, windows, True)
        idx, vals, _ = check(eng, m, windows, 15, True, payloads, tallies)
        for i in range(60):
            copies = [j for j in range(i % 5, 60, 5) if j != i]
            assert list(idx[i, 0, :11]) == copies and (vals[i, 0, :11] == 0).all(), (m, i)


def test_nan_sorts_last_inf_before_it_and_an_empty_window(eng):
    codes = random_alignment(20, 300, seed=73, divergence=0.1)
    codes[[3, 7], 100:200] = N          # raw: no site to compare in [100, 200) -> NaN
    codes[:, :4] = A                    # window [0, 4): jc69 0 for most,
    codes[1, :3] = Cc                   #   p = 3/4 -> +inf against the others,
    codes[2, :4] = Cc                   #   p = 1 -> NaN
    windows = np.array([(100, 200), (0, 4), (9, 9), (0, 300)], np.uint64)
    eng.set_path("auto")
    eng.upload(0, codes)
    for m in ALL:
        payloads, tallies = from_run_windows(eng, m, windows, True)
        check(eng, m, windows, 19, True, payloads, tallies)
    idx, vals = eng.nearest_windows("raw", windows, 19)
    for i in range(20):
        if i not in (3, 7):
            assert list(idx[i, 0, -2:]) == [3, 7] and np.isnan(vals[i, 0, -2:]).all() and not np.isnan(vals[i, 0, :-2]).any()
        assert list(idx[i, 2]) == [j for j in range(20) if j != i] and np.isnan(vals[i, 2]).all()   # the empty window
    assert np.isnan(vals[3, 0]).all() and list(idx[3, 0]) == [j for j in range(20) if j != 3]
    idx, vals = eng.nearest_windows("jc69", windows, 19)
    assert list(idx[0, 1, -2:]) == [1, 2] and np.isposinf(vals[0, 1, -2]) and np.isnan(vals[0, 1, -1])
    assert (vals[0, 1, :-2] == 0).all()
    idx, vals = eng.nearest_windows("n", windows, 19)
    assert (vals[:, 2] == 0).all() and list(idx[5, 2]) == [j for j in range(20) if j != 5]


# ---- 5. column and list edges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cols", [1, 63, 64, 65, 255, 256, 257, 513])
def test_column_edges(eng, n_cols):
    length = 260
    rows = random_alignment(3, length, seed=80, divergence=0.3)
    cols = random_alignment(n_cols, length, seed=81 + n_cols, divergence=0.3, root=rows[0])
    windows = np.array([(0, length), (100, 229), (128, 256)], np.uint64)
    eng.set_path("auto")
    eng.upload(0, rows)
    eng.upload(1, cols)
    for m in ALL:
        payloads, tallies = from_run_windows(eng, m, windows, False)
        for k in (1, 64, 256):
            idx, _, _ = check(eng, m, windows, k, False, payloads, tallies)
            assert idx.shape[2] == min(k, n_cols)   # (k above the candidates: all of them, in order)
    if n_cols >= 2:
        # the square of the column set: n_cols - 1 candidates (k = 256 at 257 candidates for 258 records comes below)
        eng.upload(0, cols)
        payloads, tallies = from_run_windows(eng, "k80", windows, True)
        idx, _, _ = check(eng, "k80", windows, 256, True, payloads, tallies, rb=max(n_cols - 5, 0), re=n_cols)
        assert idx.shape[2] == min(256, n_cols - 1)


def test_k_256_at_257_candidates(eng):
    codes = random_alignment(258, 200, seed=83, divergence=0.3)
    windows = np.array([(0, 200), (64, 192)], np.uint64)
    eng.set_path("auto")
    eng.upload(0, codes)
    for m in ("n", "tn93"):
        payloads, tallies = from_run_windows(eng, m, windows, True)
        idx, _, _ = check(eng, m, windows, 256, True, payloads, tallies)
        assert idx.shape == (258, 2, 256)


# ---- 6. the result does not depend on the slabs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("square", [False, True])
def test_slab_independence(eng, square):
    cols = random_alignment(300, 500, seed=90, divergence=0.2)
    rows = random_alignment(4, 500, seed=91, divergence=0.2, root=cols[0])
    windows = np.array([(0, 500), (0, 128), (100, 300), (300, 300), (250, 500)], np.uint64)
    eng.set_path("auto")
    eng.upload(0, cols if square else rows)
    eng.upload(1, cols)
    rb, re = (10, 14) if square else (0, 4)
    for m in ("n", "k80", "tn93"):
        first = None
        for max_entries in (0, 1, 300, 901, 1500, 2700):   # 2700: nine lists, slabs of 4 rows x 2 windows
            got = eng.nearest_windows(m, windows, 7, square=square, row_begin=rb, row_end=re, tallies=True, max_entries=max_entries)
            assert got[0].shape == (4, 5, 7)
            if first is None:
                first = got
                payloads, tallies = from_run_windows(eng, m, windows, square)
                check(eng, m, windows, 7, square, payloads, tallies, rb, re)
            assert all(bits(a).tobytes() == bits(b).tobytes() for a, b in zip(got, first)), (m, square, max_entries)


# ---- 7. more windows than a grid axis holds ------------------------------------------------------------------------------------------
def test_65536_windows(eng):
    length = 300
    row = uniform_codes(1, length, seed=9)
    cols = uniform_codes(3, length, seed=10)
    rng = np.random.default_rng(9)
    b = rng.integers(0, length + 1, da.WINDOWS_MAX)
    windows = np.stack([b, b + rng.integers(0, length + 1 - b)], axis=1).astype(np.uint64)
    eng.set_path("auto")
    eng.upload(0, row)
    eng.upload(1, cols)
    for m in ("n", "tn93"):
        payloads, tallies = from_run_windows(eng, m, windows, False)
        idx, _, _ = check(eng, m, windows, 2, False, payloads, tallies)
        assert idx.shape == (1, 65536, 2)
        check(eng, m, windows, 2, False, payloads, tallies, max_entries=3 * 40_000)   # the windows cut, too
    with pytest.raises(da.DistanceError) as e:
        eng.nearest_windows("n", np.concatenate([windows, windows[:1]]), 2, square=False)
    assert e.value.status == ERR_ARG and "65,536" in e.value.message


# ---- 8. tallies past 16 bits ---------------------------------------------------------------------------------------------------------
def test_wide_tallies(eng):
    length = 70_000
    rng = np.random.default_rng(12)
    rows = np.empty((3, length), np.uint8)
    cols = np.empty((5, length), np.uint8)
    rows[0], rows[1], rows[2] = A, Cc, rng.choice(np.array([A, Cc], np.uint8), length)
    cols[0], cols[1], cols[2], cols[3] = Cc, G, A, T
    cols[4] = rng.choice(np.array([A, G], np.uint8), length)
    windows = np.array([(0, 70_000), (1, 65_537)], np.uint64)
    eng.set_path("auto")
    eng.upload(0, rows)
    eng.upload(1, cols)
    for m in ("n", "raw", "tn93"):
        if m == "tn93":
            payloads, tallies = from_run_windows(eng, m, windows, False)
        else:
            payloads = oracle_payloads(m, rows, cols, windows)
            tallies = full_rect(expected_tallies(m, rows, cols, windows), 3, 5)
        idx, vals, tal = check(eng, m, windows, 5, False, payloads, tallies)
        assert int(tal.max()) > 65_535
    idx, vals = eng.nearest_windows("n", windows, 2, square=False)
    assert idx[0].tolist() == [[2, 4], [2, 4]] and vals[0, 0, 0] == 0 and vals[1].tolist() == [[0, 70_000], [0, 65_536]]


# ---- 9. state ------------------------------------------------------------------------------------------------------------------------
def test_deferred_planes_and_untouched_state():
    n, length = 1100, 3333
    rng = np.random.default_rng(31)
    codes = synth.alignment(synth.SEED ^ 31, n, length)
    for r in rng.choice(n, 50, replace=False):
        at = rng.choice(length, 20, replace=False)
        codes[r, at] = CODES[rng.integers(0, 17, len(at))]
    windows = np.array([(0, length), (100, 1100), (127, 129), (3332, 3333), (500, 500)], np.uint64)
    with da.Engine(0) as dense, da.Engine(0) as lazy:
        dense.set_path("dense")
        dense.upload(0, codes)
        assert dense.planes_stored(0)
        lazy.set_prep_threshold(0)
        lazy.upload(0, codes)
        assert not lazy.planes_stored(0), "the upload stored every plane: nothing here tests the deferred form"
        lazy.set_path("consensus")
        before = {m: lazy.run_square(m, 0, 40) for m in ("n", "tn93")}
        launch, path = lazy.last_launch(), lazy.last_path()
        assert not lazy.planes_stored(0)
        for m in ALL:
            got = lazy.nearest_windows(m, windows, 4, row_begin=3, row_end=30, tallies=True)
            want = dense.nearest_windows(m, windows, 4, row_begin=3, row_end=30, tallies=True)
            assert all(bits(a).tobytes() == bits(b).tobytes() for a, b in zip(got, want)), m
            assert lazy.planes_stored(0)
            assert lazy.last_launch() == launch and lazy.last_path() == path, m
        payloads = oracle_payloads("raw", codes[3:30], codes, windows)
        assert np.array_equal(lazy.nearest_windows("raw", windows, 4, row_begin=3, row_end=30)[0],
                              nearest(payloads, 4, square=True, row_begin=3))
        for m, v in before.items():
            assert lazy.run_square(m, 0, 40).tobytes() == v.tobytes() and lazy.last_path() == "consensus", m
            assert dense.run_square(m, 0, 40).tobytes() == v.tobytes(), m


def test_interleaved_with_nearest_and_run_windows():
    codes = random_alignment(150, 400, seed=95, divergence=0.2)
    windows = np.array([(0, 400), (64, 200), (300, 400)], np.uint64)

    def three(e, order):
        calls = {"nearest": lambda: e.nearest("tn93", 5, tallies=True),
                 "windows": lambda: (e.run_windows("tn93", windows), e.run_windows("tn93", windows, tallies=True)),
                 "mine": lambda: e.nearest_windows("tn93", windows, 5, tallies=True)}
        return {name: tuple(bits(x).tobytes() for x in calls[name]()) for name in order}

    with da.Engine(0) as e:
        e.upload(0, codes)
        first = three(e, ("nearest", "mine", "windows", "mine"))
        second = three(e, ("mine", "windows", "nearest"))
        third = three(e, ("windows", "nearest", "mine"))
        assert first == second == third
        payloads, tallies = from_run_windows(e, "tn93", windows, True)
        check(e, "tn93", windows, 5, True, payloads, tallies)


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
            eng.nearest_windows("raw", windows, 2, row_begin=0, row_end=2)
        return e.value.status, e.value.message

    try:
        for status, message in ThreadRanks(2).run(body):
            assert status == ERR_STATE and "dst_upload_shared runs on the consensus path only" in message
    finally:
        hip.lib.hipFree(d_codes)


# ---- 10. capacity and errors --------------------------------------------------------------------------------------------------------
def test_capacity_and_errors():
    codes = uniform_codes(9, 200, seed=5)
    windows = np.array([(0, 200), (10, 20), (199, 200)], np.uint64)
    lib = da.load()
    guard = 16
    FILL = 0xABABABAB
    with da.Engine(0) as eng:
        h = eng._h

        def call(measure=2, square=1, rs=0, cs=1, rb=0, re=9, wb=windows[:, 0], we=windows[:, 1], nw=3, k=4, cap=None, index=True,
                 k_used=True, entries=9 * 3 * 4):
            idx = np.full(entries + 2 * guard, FILL, np.uint32)
            val = np.full(entries + 2 * guard, FILL, np.uint64)
            tal = np.full((entries + 2 * guard) * 2, FILL, np.uint32)
            wb = None if wb is None else np.ascontiguousarray(wb)
            we = None if we is None else np.ascontiguousarray(we)
            ku = C.c_uint32(77)
            rc = lib.dst_nearest_windows(h, measure, square, rs, cs, rb, re, None if wb is None else wb.ctypes.data,
                                         None if we is None else we.ctypes.data, nw, k, 0,
                                         idx[guard:].ctypes.data if index else None, tal[2 * guard:].ctypes.data,
                                         val[guard:].ctypes.data, entries if cap is None else cap, C.byref(ku) if k_used else None)
            untouched = bool((idx == FILL).all() and (val == FILL).all() and (tal == FILL).all())
            return rc, ku.value, untouched, (idx, val, tal), eng._lib.dst_last_error(h).decode()

        rc, ku, untouched, _, msg = call()
        assert rc == ERR_STATE and msg == "set not uploaded" and ku == 0 and untouched
        eng.upload(0, codes)
        payloads, tallies = from_run_windows(eng, "raw", windows, True)
        rc, ku, untouched, (idx, val, tal), _ = call()
        assert rc == 0 and ku == 4 and not untouched
        want = nearest(payloads, 4, square=True)
        assert np.array_equal(idx[guard:guard + 108].reshape(9, 3, 4), want)
        assert np.array_equal(val[guard:guard + 108].reshape(9, 3, 4), bits(take(payloads, want)))
        assert np.array_equal(tal[2 * guard:2 * guard + 216].reshape(9, 3, 4, 2), take(tallies, want))
        assert (idx[:guard] == FILL).all() and (idx[guard + 108:] == FILL).all() and (tal[2 * guard + 216:] == FILL).all()
        # capacity: nothing written, *k_used says what the entries would be
        rc, ku, untouched, _, msg = call(cap=107)
        assert rc == ERR_CAPACITY and untouched and ku == 4 and "cap_entries" in msg
        rc, ku, untouched, _, _ = call(k=200, cap=9 * 3 * 8 - 1)   # k above the 8 candidates
        assert rc == ERR_CAPACITY and untouched and ku == 8
        # DST_OK, nothing written, *k_used set: no window, an empty row range
        for kw in (dict(nw=0), dict(rb=4, re=4), dict(rb=9, re=9)):
            rc, ku, untouched, _, _ = call(**kw)
            assert rc == 0 and untouched and ku == 4, kw
        bad = [
            (dict(nw=da.WINDOWS_MAX + 1), "more than DST_WINDOWS_MAX"), (dict(nw=da.WINDOWS_MAX + 1, wb=None, measure=9, k=0), "more than"),
            (dict(wb=None), "null pointer"), (dict(we=None, measure=9), "null pointer"),
            (dict(measure=6, k=0), "unknown measure"), (dict(measure=-1), "unknown measure"),
            (dict(k=0, index=False), "k must be between 1 and 256"), (dict(k=257), "k must be between 1 and 256"),
            (dict(index=False, square=0, rs=0, cs=0), "null index or k_used pointer"), (dict(k_used=False), "null index or k_used pointer"),
            (dict(square=0, rs=0, cs=0, rb=5, re=4), "row_slot == col_slot"), (dict(square=0, rs=0, cs=2), "slot must be 0 or 1"),
            (dict(square=0, rs=-1, cs=0), "slot must be 0 or 1"),
            (dict(wb=np.array([0, 21, 5], np.uint64), rb=5, re=4), "window 1 [21, 20)"),
            (dict(we=np.array([200, 20, 201], np.uint64)), "window 2 [199, 201)"),
            (dict(rb=5, re=4), "row range out of bounds"), (dict(re=10), "row range out of bounds"),
        ]
        for kw, text in bad:
            rc, ku, untouched, _, msg = call(**kw)
            assert rc == ERR_ARG and text in msg and untouched and ku in (0, 77), (kw, rc, msg)
        rc, _, untouched, _, msg = call(square=0, rs=0, cs=1, wb=np.array([0, 21, 5], np.uint64))
        assert rc == ERR_STATE and msg == "set not uploaded" and untouched
        eng.upload(1, uniform_codes(5, 90, seed=6))
        rc, _, untouched, _, msg = call(square=0, rs=0, cs=1)
        assert rc == ERR_STATE and "Different length sequences" in msg and untouched
        # no candidates: a square set of one record (an empty set cannot be uploaded)
        eng.upload(0, codes[:1])
        rc, ku, untouched, _, _ = call(re=1)
        assert rc == 0 and ku == 0 and untouched
        # after the errors the context still answers
        eng.upload(0, codes)
        assert np.array_equal(eng.nearest_windows("raw", windows, 4)[0], want)
