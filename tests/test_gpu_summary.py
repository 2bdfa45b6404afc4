"""GPU (-m gpu): dst_summary / Engine.summary, the per-record and histogram summaries of the pairwise distances — exact
against the numpy / Python-integer restatement of the definition (summary_reference) applied to the context's own
run_square / run_rect values, integers equal and sums bitwise: every measure on every kernel path, the rectangle, any slab
bound, the kernels' boundaries, NaN / +inf / -0.0, concentrated and spread histograms, tiny sets, every error status and
the state a call leaves behind."""
import ctypes as C

import numpy as np
import pytest

import distance_amd as da
from helpers import CODES, KNOWN, LETTERS, random_alignment, uniform_codes
from summary_reference import assert_summary, hist_of, rethreshold, summary
from test_gpu_links import datasets, interior, median

pytestmark = pytest.mark.gpu
ALL = ("n", "n_high", "raw", "jc69", "k80", "tn93")
ERR_ARG, ERR_STATE, ERR_CAPACITY = 1, 4, 6
INF = float("inf")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def finite_max(vals):
    v = vals[np.isfinite(vals)] if vals.dtype == np.float64 else vals
    return float(v.max()) if len(v) else 0.0


def width_for(m, vals, parts):
    """(largest finite value) / parts as a valid width: an integer >= 1 for the int measures"""
    w = finite_max(vals) / parts
    if m in da.INT_MEASURES:
        return float(max(int(w), 1))
    return w if w > 0 else 1.0


def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and np.array_equal(bits(a[k]) if a[k].dtype.itemsize == 8 else a[k],
                                                               bits(b[k]) if b[k].dtype.itemsize == 8 else b[k]), k
        else:
            assert bits(np.float64(a[k])) == bits(np.float64(b[k])) if isinstance(a[k], float) else a[k] == b[k], k


@pytest.fixture(scope="module")
def sets():
    return datasets()


def test_status_codes_are_the_headers():
    text = open(da._lib.HEADER_PATH).read()
    for name, value in (("DST_ERR_ARG", ERR_ARG), ("DST_ERR_CAPACITY", ERR_CAPACITY), ("DST_ERR_STATE", ERR_STATE)):
        assert f"{name} = {value}" in text or f"{name} {value}" in text, name


# ---- 1. every measure on every path -------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["dense", "consensus", "hybrid"])
@pytest.mark.parametrize("kind", ["low", "clade", "nrun", "uniform"])
def test_every_measure_every_path(sets, path, kind):
    codes = sets[kind]
    n = len(codes)
    with da.Engine(0) as eng:
        eng.set_prep_threshold(0)
        eng.set_path(path)
        eng.upload(0, codes)
        for m in ALL:
            vals = eng.run_square(m)
            w50, w100 = width_for(m, vals, 50), width_for(m, vals, 100)
            base = summary(m, vals, n, n, True, 0.0, bins=64, width=w50)
            for t in (0.0, interior(vals), median(vals), INF):
                what = (path, kind, m, t)
                want = rethreshold(base, m, vals, n, n, True, t)
                got = eng.summary(m, t, bins=64, width=w50)
                assert_summary(got, want, what)
                assert got["links"] == eng.clusters(m, t)[1] == eng.links(m, t, count_only=True), what
                row, col = eng.links(m, t, values=False)
                deg = np.bincount(row, minlength=n) + np.bincount(col, minlength=n)
                assert np.array_equal(got["within"], deg.astype(np.uint32)), what
            # the open last bin in use (values up to 100 widths, 64 bins), without the per-record passes
            got = eng.summary(m, 0.0, bins=64, width=w100, per_record=False)
            assert "within" not in got and "sum" not in got
            assert_summary(got, dict(base, hist=hist_of(m, vals, 64, w100)), (path, kind, m, "w100"))
            assert got["hist"][63] > 0 or finite_max(vals) < 63 * w100
            if m in da.INT_MEASURES:
                got = eng.summary(m, 0.0, bins=64, width=1, per_record=False)
                assert_summary(got, dict(base, hist=hist_of(m, vals, 64, 1.0)), (path, kind, m, "width 1"))
            # no histogram: the per-record passes alone
            got = eng.summary(m, 0.0)
            assert "hist" not in got
            assert_summary(got, base, (path, kind, m, "no hist"))


# ---- 2. the rectangle -----------------------------------------------------------------------------------------------------
def test_rectangle_both_orders():
    codes = random_alignment(338, 200, seed=91)
    a, b = np.ascontiguousarray(codes[:37]), np.ascontiguousarray(codes[37:])
    with da.Engine(0) as eng:
        eng.upload(0, a)
        eng.upload(1, b)
        for rs, cs, nr, nc in ((0, 1, 37, 301), (1, 0, 301, 37)):
            for m in ALL:
                vals = eng.run_rect(m, rs, cs)
                w = width_for(m, vals.reshape(-1), 50)
                base = summary(m, vals, nr, nc, False, 0.0, bins=64, width=w)
                for t in (0.0, interior(vals.reshape(-1)), INF):
                    want = rethreshold(base, m, vals, nr, nc, False, t)
                    got = eng.summary(m, t, square=False, row_slot=rs, col_slot=cs, bins=64, width=w)
                    assert len(got["within"]) == nr
                    assert_summary(got, want, (rs, cs, m, t))
                    assert got["links"] == eng.links(m, t, square=False, row_slot=rs, col_slot=cs, count_only=True)
                    row, _ = eng.links(m, t, square=False, row_slot=rs, col_slot=cs, values=False)
                    assert np.array_equal(got["within"], np.bincount(row, minlength=nr).astype(np.uint32))
                only = eng.summary(m, INF, square=False, row_slot=rs, col_slot=cs, per_record=False)   # the totals alone
                assert_summary(only, rethreshold(base, m, vals, nr, nc, False, INF), (rs, cs, m, "totals"))
        for s in (0, 1):
            with pytest.raises(da.DistanceError) as e:
                eng.summary("raw", 1.0, square=False, row_slot=s, col_slot=s)
            assert e.value.status == ERR_ARG and "use the square form" in e.value.message


# ---- 3. the slab bound does not change the result ----------------------------------------------------------------------
def test_slab_sizes(sets):
    codes = sets["clade"]
    n = len(codes)
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        eng.upload(1, np.ascontiguousarray(sets["low"][:41]))
        for square, nr, nc in ((True, n, n), (False, n, 41)):
            for m in ("n_high", "raw", "tn93"):
                vals = eng.run_square(m) if square else eng.run_rect(m, 0, 1)
                t, w = median(vals.reshape(-1)), width_for(m, vals.reshape(-1), 50)
                want = summary(m, vals, nr, nc, square, t, bins=64, width=w)
                first = None
                for max_pairs in (1, 300, n - 1, n, 0):
                    got = eng.summary(m, t, square=square, max_pairs=max_pairs, bins=64, width=w)
                    assert_summary(got, want, (square, m, max_pairs))
                    first = first or got
                    same(got, first)


# ---- 4. the kernels' boundaries ----------------------------------------------------------------------------------------
def test_row_runs_and_column_segments():
    """2,051 records: rows of 2,050 / 2,049 / 2,048 / 2,047 entries cross the 2048-entry run of a workgroup of the row pass;
    the slab's rows cross the 64-row segments of the column pass, at the default slab bound and at bounds that end a slab
    inside a segment."""
    n = 2051
    codes = uniform_codes(n, 64, seed=41)
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        for m in ("n_high", "raw"):
            vals = eng.run_square(m)
            t, w = median(vals), width_for(m, vals, 50)
            want = summary(m, vals, n, n, True, t, bins=64, width=w)
            for max_pairs in (0, 65 * n, 100_000):
                assert_summary(eng.summary(m, t, max_pairs=max_pairs, bins=64, width=w), want, (m, max_pairs))
            assert want["within"].sum() == 2 * want["links"] and want["links"] > 0


def test_two_row_grids():
    """65,537 row records against 2: the row pass takes two grids (65,535 rows each at most)."""
    nr = 65537
    codes = uniform_codes(nr + 2, 16, seed=42)
    with da.Engine(0) as eng:
        eng.upload(0, np.ascontiguousarray(codes[:nr]))
        eng.upload(1, np.ascontiguousarray(codes[nr:]))
        for m in ("n", "jc69"):
            vals = eng.run_rect(m, 0, 1)
            t, w = median(vals.reshape(-1)), width_for(m, vals.reshape(-1), 10)
            want = summary(m, vals, nr, 2, False, t, bins=16, width=w)
            assert_summary(eng.summary(m, t, square=False, bins=16, width=w), want, m)
            if m == "n":
                assert list(want["summable"][65535:]) == [2, 2]   # (the second grid's rows count)


def test_histogram_sizes():
    codes = random_alignment(90, 300, seed=43, divergence=0.2)
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        for m in ("n_high", "tn93"):
            vals = eng.run_square(m)
            base = summary(m, vals, 90, 90, True, 0.0)
            for bins, parts in ((1, 3), (4096, 4000), (4096, 5000), (7, 7)):
                w = width_for(m, vals, parts)
                got = eng.summary(m, 0.0, bins=bins, width=w, per_record=False)
                assert_summary(got, dict(base, hist=hist_of(m, vals, bins, w)), (m, bins, parts))
        # a slab with fewer entries than one workgroup has threads: 5 records, 10 pairs, and one row per slab
        eng.upload(0, np.ascontiguousarray(codes[:5]))
        for m in ("n", "raw"):
            vals = eng.run_square(m)
            w = width_for(m, vals, 4)
            want = summary(m, vals, 5, 5, True, 0.0, bins=5, width=w)
            for max_pairs in (0, 1):
                assert_summary(eng.summary(m, 0.0, bins=5, width=w, max_pairs=max_pairs), want, (m, max_pairs))


def test_bin_edges_on_the_device():
    """n_high values 0 .. 39 at widths whose multiples they hit exactly (k width_q and k width_q - 1 side by side)."""
    codes = spread_codes(200)
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        vals = eng.run_square("n_high")
        assert set(np.unique(vals)) == set(range(40))
        base = summary("n_high", vals, 200, 200, True, 0.0)
        for bins, w in ((64, 1.0), (40, 1.0), (39, 1.0), (13, 3.0), (14, 3.0), (4, 13.0), (2, 39.0), (2, 40.0)):
            got = eng.summary("n_high", 0.0, bins=bins, width=w, per_record=False)
            assert_summary(got, dict(base, hist=hist_of("n_high", vals, bins, w)), (bins, w))
        raw = eng.run_square("raw")   # k / 64: every value a multiple of the width 1 / 64 and of 3 / 64
        base = summary("raw", raw, 200, 200, True, 0.0)
        for bins, w in ((64, 1 / 64), (40, 1 / 64), (20, 3 / 64), (4096, 2.0 ** -20), (5, 0.1)):
            got = eng.summary("raw", 0.0, bins=bins, width=w, per_record=False)
            assert_summary(got, dict(base, hist=hist_of("raw", raw, bins, w)), (bins, w))


# ---- 5. designed values ------------------------------------------------------------------------------------------------
def encode(text):
    lut = {LETTERS[k]: int(c) for k, c in enumerate(CODES)}
    return np.array([lut[c] for c in text], np.uint8)


def test_nan_pairs():
    codes = random_alignment(30, 100, seed=94)
    codes[3] = 240
    codes[7] = 240   # two all-N records: every pair with one of them is 0 / 0
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        vals = eng.run_square("raw")
        assert np.isnan(vals).sum() == 2 * 28 + 1
        w = width_for("raw", vals, 10)
        for t in (0.0, 0.5, INF):
            got = eng.summary("raw", t, bins=16, width=w)
            assert_summary(got, summary("raw", vals, 30, 30, True, t, bins=16, width=w), t)
            assert got["nan_pairs"] == 57 and int(got["hist"].sum()) == got["pairs"] - 57 == got["summable_pairs"]
            for x in (3, 7):   # every partner NaN: nothing within, nothing summable, a zero sum
                assert got["within"][x] == 0 and got["summable"][x] == 0 and bits(got["sum"][x:x + 1])[0] == 0
            assert all(got["summable"][x] == 27 for x in range(30) if x not in (3, 7))
        only = eng.summary("raw", INF, per_record=False)
        assert only["nan_pairs"] == 57 and only["links"] == len(vals) - 57


def test_negative_zero_and_infinity():
    a = b"ACGTACGTACGTACGTAAAA"
    rows = [a, a, b"CATGCATGCATGCATTAAAA",    # 15 of 20 sites differ from a: p = 0.75, jc69 +inf
            b"GTACGTACGTGTACGTAAAA",          # 10 of 20 sites are transitions of a: P = 0.5, Q = 0, k80 +inf
            b"CATGCATGCATGCATGAAAA"]          # p = 0.8: NaN
    codes = np.stack([encode(r) for r in rows])
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        for m in ("jc69", "k80"):
            vals = eng.run_square(m)
            assert vals[0] == 0.0 and np.signbit(vals[0]), m   # the pair (0, 1): -0.0
            n_inf, n_nan = int(np.isposinf(vals).sum()), int(np.isnan(vals).sum())
            assert n_inf and n_nan
            for t in (0.0, -0.0, 1e308, INF):
                got = eng.summary(m, t, bins=8, width=0.5)
                assert_summary(got, summary(m, vals, 5, 5, True, t, bins=8, width=0.5), (m, t))
            # +inf: in the last bin, not summable, not in the sum; NaN: in nan_pairs and nowhere else
            assert got["hist"][7] >= n_inf and got["nan_pairs"] == n_nan and int(got["hist"].sum()) == 10 - n_nan
            assert got["summable_pairs"] == 10 - n_nan - n_inf and got["links"] == 10 - n_nan
            assert np.isfinite(got["sum"]).all() and np.isfinite(got["total_sum"])
            zero = eng.summary(m, 0.0)
            assert zero["links"] == 1 and list(zero["within"]) == [1, 1, 0, 0, 0]   # -0.0 links at T = 0.0


def test_identical_records():
    """300 identical records: every pair falls into bin 0 (the wave-aggregated path of the histogram pass takes all of it)."""
    n = 300
    codes = np.repeat(random_alignment(1, 500, seed=44), n, axis=0)
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        for m in ALL:
            vals = eng.run_square(m)
            w = 1.0 if m in da.INT_MEASURES else 0.001
            got = eng.summary(m, 0.0, bins=256, width=w)
            assert_summary(got, summary(m, vals, n, n, True, 0.0, bins=256, width=w), m)
            assert got["hist"][0] == n * (n - 1) // 2 == got["links"] and not got["hist"][1:].any()
            assert np.all(got["within"] == n - 1) and np.all(got["summable"] == n - 1) and not got["sum"].any()


def spread_codes(n, L=64):
    """record j = a base with its first j mod 40 sites changed A -> C: n(i, j) = |i mod 40 - j mod 40|, so consecutive
    entries of a row fall into different bins at width 1 (the histogram pass' fall-through path)."""
    codes = np.full((n, L), KNOWN[0], np.uint8)
    for j in range(n):
        codes[j, :j % 40] = KNOWN[2]
    return codes


def test_spread_histogram():
    n = 500
    codes = spread_codes(n)
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        for m in ("n", "raw"):
            vals = eng.run_square(m)
            w = 1.0 if m == "n" else 1.0 / 64
            got = eng.summary(m, 3.0 if m == "n" else 3.0 / 64, bins=48, width=w)
            want = summary(m, vals, n, n, True, 3.0 if m == "n" else 3.0 / 64, bins=48, width=w)
            assert_summary(got, want, m)
            assert (got["hist"][:40] > 0).all() and not got["hist"][40:].any()
            assert np.mean(np.diff(vals[:n - 1]) != 0) > 0.9   # row 0: neighbours differ


# ---- 7. tiny sets, errors, state ---------------------------------------------------------------------------------------
def test_tiny_sets():
    codes = random_alignment(3, 50, seed=95, divergence=0.3)
    with da.Engine(0) as eng:
        with pytest.raises(da.DistanceError):
            eng.upload(0, codes[:0])   # (an empty set is not accepted by upload: n = 0 and an empty rectangle side cannot arise)
        eng.upload(0, codes[:1])
        got = eng.summary("raw", INF, bins=4, width=0.5)
        assert got["pairs"] == got["nan_pairs"] == got["summable_pairs"] == got["links"] == 0 and got["total_sum"] == 0.0
        assert list(got["within"]) == [0] and list(got["summable"]) == [0] and list(got["sum"]) == [0.0] and list(got["hist"]) == [0] * 4
        eng.upload(0, np.ascontiguousarray(codes[[0, 0]]))
        got = eng.summary("raw", 0.0, bins=4, width=0.5)
        assert got["pairs"] == 1 and got["links"] == 1 and list(got["within"]) == [1, 1] and list(got["hist"]) == [1, 0, 0, 0]
        eng.upload(0, codes[:2])
        eng.upload(1, codes[2:3])   # a rectangle of 2 x 1 and 1 x 2
        for m in ("n", "tn93"):
            vals = eng.run_square(m)
            assert_summary(eng.summary(m, INF, bins=3, width=width_for(m, vals, 2)),
                           summary(m, vals, 2, 2, True, INF, bins=3, width=width_for(m, vals, 2)), m)
            for rs, cs in ((0, 1), (1, 0)):
                vals = eng.run_rect(m, rs, cs)
                w = width_for(m, vals.reshape(-1), 2)
                assert_summary(eng.summary(m, INF, square=False, row_slot=rs, col_slot=cs, bins=3, width=w),
                               summary(m, vals, vals.shape[0], vals.shape[1], False, INF, bins=3, width=w), (m, rs, cs))


def test_errors():
    lib = da.load()
    codes = random_alignment(50, 100, seed=96)
    hist = np.full(8, 7, np.uint64)
    within, summable, sums = np.full(50, 7, np.uint32), np.full(50, 7, np.uint32), np.full(50, 7.0)
    tot = da._lib.SummaryTotals()

    def call(h, m=2, square=1, rs=0, cs=1, t=1.0, bins=8, width=0.1, hp=hist.ctypes.data, cap=50, per_record=True):
        tot.pairs = 99
        return lib.dst_summary(h, m, square, rs, cs, t, 0, bins, width, hp, within.ctypes.data if per_record else None,
                               summable.ctypes.data if per_record else None, sums.ctypes.data if per_record else None, cap,
                               C.byref(tot))

    with da.Engine(0) as eng:
        h = eng._h
        assert call(h) == ERR_STATE and tot.pairs == 0 and b"not uploaded" in lib.dst_last_error(h)
        eng.upload(0, codes)
        assert call(h, square=0) == ERR_STATE   # slot 1 is empty
        assert call(h, t=float("nan")) == ERR_ARG and b"threshold is NaN" in lib.dst_last_error(h) and tot.pairs == 0
        assert call(h, m=9) == ERR_ARG and call(h, m=-1) == ERR_ARG and b"unknown measure" in lib.dst_last_error(h)
        assert call(h, bins=4097) == ERR_ARG and call(h, hp=None) == ERR_ARG
        for width in (0.0, -1.0, float("nan"), INF, 2.0 ** 25, 2.0 ** -39):
            assert call(h, width=width) == ERR_ARG, width
        assert call(h, width=2.0 ** -38 * 1.5) == 0   # width_q = rint(0.75) = 1
        for width in (0.5, 2.5, 0.0):
            assert call(h, m=0, width=width) == ERR_ARG and call(h, m=1, width=width) == ERR_ARG, width
        assert call(h, bins=0, width=float("nan"), hp=None) == 0   # without a histogram the width means nothing
        assert call(h, square=0, rs=2) == ERR_ARG and call(h, square=0, cs=-1) == ERR_ARG
        assert call(h, square=0, rs=1, cs=1) == ERR_ARG and b"use the square form" in lib.dst_last_error(h)
        assert call(h, cap=49) == ERR_CAPACITY and call(h, cap=49, per_record=False) == 0
        eng.upload(1, random_alignment(5, 90, seed=97))
        assert call(h, square=0) == ERR_STATE and b"Different length sequences" in lib.dst_last_error(h)
        assert call(h, t=INF) == 0 and tot.pairs == 50 * 49 // 2 and int(hist.sum()) + tot.nan_pairs == tot.pairs
        assert lib.dst_summary(h, 2, 1, 0, 1, INF, 0, 0, 0.0, None, within.ctypes.data, None, None, 50, None) == 0   # totals NULL
        assert int(within.sum()) == 2 * tot.links
        assert lib.dst_summary(h, 2, 1, 0, 1, INF, 0, 0, 0.0, None, None, None, None, 0, None) == 0   # nothing asked for


@pytest.mark.parametrize("path", ["auto", "dense", "consensus"])
def test_run_square_unchanged(sets, path):
    codes = sets["nrun"]
    with da.Engine(0) as eng:
        eng.set_prep_threshold(0)
        eng.set_path(path)
        eng.upload(0, codes)
        for m in ("raw", "tn93"):
            before = eng.run_square(m)
            used = eng.last_path()
            eng.summary(m, interior(before), max_pairs=2000, bins=32, width=width_for(m, before, 30))
            eng.summary(m, 0.0, per_record=False)
            after = eng.run_square(m)
            assert np.array_equal(bits(before), bits(after)) and eng.last_path() == used, (path, m)


def test_between_the_other_analyses(sets):
    """The slab scratch is shared: summaries between the other analyses, each result that of the first call."""
    codes = sets["clade"]
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        first = {m: eng.summary(m, t, bins=40, width=w) for m, t, w in (("tn93", 0.002, 0.0005), ("n_high", 3.0, 2.0))}
        for other in (lambda: eng.clusters("n_high", 3.0, max_pairs=500), lambda: eng.links("tn93", 0.002, max_pairs=500, tallies=True),
                      lambda: eng.nearest("tn93", k=3, tallies=True), lambda: eng.mst("raw", max_pairs=500)):
            other()
            same(eng.summary("tn93", 0.002, bins=40, width=0.0005, max_pairs=700), first["tn93"])
            same(eng.summary("n_high", 3.0, bins=40, width=2.0), first["n_high"])
