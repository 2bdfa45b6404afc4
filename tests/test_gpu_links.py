"""GPU (-m gpu): dst_links / Engine.links, the pairs within a threshold in canonical pair order — exact against the numpy
restatement of the link rule (links_reference) applied to the context's own run_square / run_rect values: every measure on
every kernel path, the rectangle, any slab bound, links placed on the kernels' boundaries, a slab with more links than one
sink call carries, NaN / -0.0 / +inf, tiny sets, every error status, the state a call leaves behind, and one full-size set."""
import ctypes as C

import numpy as np
import pytest

import distance_amd as da
from helpers import CODES, KNOWN, LETTERS, random_alignment, uniform_codes
from links_reference import components, expected, linked
from tools import synth

pytestmark = pytest.mark.gpu
ALL = ("n", "n_high", "raw", "jc69", "k80", "tn93")
ERR_ARG, ERR_STATE = 1, 4
INF = float("inf")
CHUNK = da.LINKS_CHUNK


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def interior(vals):
    """A threshold inside the values: the 2 % quantile of the finite ones."""
    v = vals[np.isfinite(vals)] if vals.dtype == np.float64 else vals
    return float(np.quantile(v, 0.02)) if len(v) else 0.0


def median(vals):
    v = vals[np.isfinite(vals)] if vals.dtype == np.float64 else vals
    return float(np.median(v)) if len(v) else 0.0


def assert_links(got, want, what):
    """row, col equal, values bitwise equal"""
    assert got[0].dtype == np.uint32 and got[1].dtype == np.uint32, what
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what
    assert got[2].dtype == want[2].dtype and np.array_equal(bits(got[2]), bits(want[2])), what


def datasets():
    """the four sets of test_gpu_clusters.datasets()"""
    n, L = 260, 3000
    r = synth.root(synth.SEED, L)
    low = synth.records(synth.SEED, r, 0, n)
    clade = low.copy()
    synth.apply_clades(clade, r, *synth.clade_plan(synth.SEED, n, L))
    nrun = low.copy()
    synth.apply_nruns(nrun, synth.nrun_plan(synth.SEED, n, L, share=0.1))
    return {"low": low, "clade": clade, "nrun": nrun, "uniform": uniform_codes(120, 64, seed=5)}


@pytest.fixture(scope="module")
def sets():
    return datasets()


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
        counts = eng.base_counts(0)
        for m in ALL:
            vals = eng.run_square(m)
            tal = eng.run_square(m, tallies=True)
            for t in (0.0, interior(vals), median(vals), INF):
                what = (path, kind, m, t)
                want = expected(m, vals, n, n, True, t)
                mask = linked(m, vals, t)
                got = eng.links(m, t)
                assert len(got) == 3
                assert_links(got, want, what)
                labels, n_links = eng.clusters(m, t)
                assert len(got[0]) == n_links == eng.links(m, t, count_only=True), what
                assert np.array_equal(components(n, got[0], got[1]), labels), what
                full = eng.links(m, t, tallies=True)
                assert len(full) == 4 and full[3].dtype == np.uint32 and full[3].shape == (len(want[0]), da.tally_width(m))
                assert_links(full, want, what)
                assert np.array_equal(full[3], tal[mask]), what
                only = eng.links(m, t, values=False, tallies=True)
                assert len(only) == 3 and np.array_equal(only[0], want[0]) and np.array_equal(only[2], tal[mask]), what
                at = np.nonzero(mask)[0]
                for e in range(0, len(at), max(len(at) // 5, 1)):   # a few links through the host finalisation
                    i, j = int(full[0][e]), int(full[1][e])
                    a = da.finalize(m, full[3][e], counts[i], counts[j])   # tn93: base counts in (row, col) order
                    b = da.finalize(m, tal[at[e]], counts[i], counts[j])
                    assert a == b or (a != a and b != b), what


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
                tal = eng.run_rect(m, rs, cs, tallies=True).reshape(nr * nc, -1)
                for t in (0.0, interior(vals.reshape(-1)), INF):
                    want = expected(m, vals, nr, nc, False, t)
                    got = eng.links(m, t, square=False, row_slot=rs, col_slot=cs, tallies=True)
                    assert_links(got, want, (rs, cs, m, t))
                    assert np.array_equal(got[3], tal[linked(m, vals.reshape(-1), t)]), (rs, cs, m, t)
                    assert eng.links(m, t, square=False, row_slot=rs, col_slot=cs, count_only=True) == len(want[0])
        for s in (0, 1):
            with pytest.raises(da.DistanceError) as e:
                eng.links("raw", 1.0, square=False, row_slot=s, col_slot=s)
            assert e.value.status == ERR_ARG


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
                t = median(vals.reshape(-1))
                want = expected(m, vals, nr, nc, square, t)
                assert len(want[0]) > 1000
                tal = None
                for max_pairs in (1, n - 1, 3000, 0):   # one row per slab (1: below a row), a few thousand, the default
                    got = eng.links(m, t, square=square, max_pairs=max_pairs, tallies=True)
                    assert_links(got, want, (square, m, max_pairs))
                    tal = got[3] if tal is None else tal
                    assert np.array_equal(got[3], tal), (square, m, max_pairs)
                    calls, first = eng.last_links_calls, eng.last_links_first
                    assert all(1 <= c <= CHUNK for c in calls) and sum(calls) == len(want[0])
                    assert first == [int(x) for x in np.cumsum([0] + calls[:-1])], (square, m, max_pairs)
                    if max_pairs == 1:   # a slab is one row: one call per row that has a link
                        assert len(calls) == len(np.unique(want[0])), (square, m)


# ---- 4. links on the kernels' boundaries -------------------------------------------------------------------------------
def test_positions():
    n, L = 2600, 128
    codes = np.ascontiguousarray(np.random.default_rng(92).choice(np.array(KNOWN, np.uint8), size=(n, L)))   # high diversity
    # copies of record 0: entries 0 and n-2 of row 0 (its first and last pair), 63 / 64 (two waves' steps: lanes 63 and 0),
    # 2047 / 2048 / 2049 (the end of the row's first workgroup and the start of its second), the last row's single pair,
    # and rows 64 and 65, between which max_pairs below puts a slab boundary
    copies = [1, 64, 65, 2048, 2049, 2050, n - 2, n - 1]
    codes[copies] = codes[0]
    group = [0] + copies
    designed = sorted((a, b) for a in group for b in group if a < b)
    first_slab = sum(n - 1 - i for i in range(65))   # rows 0 .. 64 exactly
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        vals = eng.run_square("n_high")
        i, j = np.triu_indices(n, 1)
        zero = vals == 0
        assert sorted(zip(i[zero].tolist(), j[zero].tolist())) == designed   # exactly the designed pairs, on run_square alone
        for a, b in ((0, 1), (0, n - 1), (0, 64), (0, 65), (0, 2048), (0, 2049), (0, 2050), (n - 2, n - 1), (64, 65), (65, 2048)):
            assert (a, b) in designed
        ends = []
        eng.run_slabs("n_high", lambda first, rb, re, arr: ends.append(re) and False, first_slab)
        assert ends[0] == 65   # the first slab ends behind row 64: rows 64 and 65 both hold links
        for m in ("n_high", "raw"):
            v = vals if m == "n_high" else eng.run_square(m)
            want = expected(m, v, n, n, True, 0.0)
            assert sorted(zip(want[0].tolist(), want[1].tolist())) == designed
            for max_pairs in (0, first_slab, 1):
                got = eng.links(m, 0.0, max_pairs=max_pairs, tallies=True)
                assert_links(got, want, (m, max_pairs))
                assert list(zip(got[0].tolist(), got[1].tolist())) == designed
            assert eng.last_links_calls == [8, 7, 6, 5, 4, 3, 2, 1]   # (one row per slab: the rows of the group but the last)
            eng.links(m, 0.0, max_pairs=first_slab)
            assert eng.last_links_calls[0] == 8 + 7 + 6   # rows 0, 1 and 64 lie in the first slab, row 65 in the second


# ---- 5. a slab with more links than one sink call carries --------------------------------------------------------------
def test_chunk_window():
    n = 3000
    pairs = n * (n - 1) // 2
    assert pairs == 4_498_500 and pairs > CHUNK == 4_194_304
    codes = uniform_codes(n, 64, seed=93)
    i, j = np.triu_indices(n, 1)
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        vals = eng.run_square("n_high")
        got = eng.links("n_high", INF)
        assert eng.last_links_calls == [4194304, 304196] and eng.last_links_first == [0, 4194304]
        assert np.array_equal(got[0], i.astype(np.uint32)) and np.array_equal(got[1], j.astype(np.uint32))
        assert np.array_equal(got[2], vals)
        assert eng.links("n_high", INF, count_only=True) == pairs and eng.last_links_calls == []
        raw = eng.run_square("raw")
        tal = eng.run_square("raw", tallies=True)
        keep = ~np.isnan(raw)
        want = expected("raw", raw, n, n, True, INF)
        assert len(want[0]) > CHUNK
        got = eng.links("raw", INF, tallies=True)
        assert eng.last_links_calls == [CHUNK, len(want[0]) - CHUNK]
        assert_links(got, want, "raw")
        assert np.array_equal(got[3], tal[keep])
        # a window that ends inside a workgroup's run and a threshold that links about half: two windows again
        t = median(raw)
        want = expected("raw", raw, n, n, True, t)
        assert_links(eng.links("raw", t), want, "raw median")


# ---- 6. special values -------------------------------------------------------------------------------------------------
def encode(text):
    lut = {LETTERS[k]: int(c) for k, c in enumerate(CODES)}
    return np.array([lut[c] for c in text], np.uint8)


def test_nan_is_never_a_link():
    codes = random_alignment(30, 100, seed=94)
    codes[3] = 240
    codes[7] = 240   # two all-N records: every pair with one of them is 0 / 0
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        vals = eng.run_square("raw")
        nan = np.isnan(vals)
        assert nan.sum() == 2 * 28 + 1
        for t in (0.0, 0.5, INF):
            want = expected("raw", vals, 30, 30, True, t)
            got = eng.links("raw", t)
            assert_links(got, want, t)
            assert not np.isin(got[0], (3, 7)).any() and not np.isin(got[1], (3, 7)).any()
        assert eng.links("raw", INF, count_only=True) == int((~nan).sum())


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
            assert np.isposinf(vals).any() and np.isnan(vals).any(), (m, vals)
            got = eng.links(m, 0.0)
            assert_links(got, expected(m, vals, 5, 5, True, 0.0), m)
            assert list(zip(got[0], got[1])) == [(0, 1)] and np.signbit(got[2][0])   # -0.0 links at T = 0.0, as itself
            assert_links(eng.links(m, -0.0), expected(m, vals, 5, 5, True, 0.0), m)
            big = eng.links(m, 1e308)
            assert not np.isinf(big[2]).any() and len(big[0]) == int(np.isfinite(vals).sum())
            top = eng.links(m, INF)   # +inf links only at T = inf
            assert_links(top, expected(m, vals, 5, 5, True, INF), m)
            assert int(np.isposinf(top[2]).sum()) == int(np.isposinf(vals).sum()) and not np.isnan(top[2]).any()


def test_integer_thresholds(sets):
    codes = sets["low"]
    n = len(codes)
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        for m in ("n", "n_high"):
            vals = eng.run_square(m)
            t = float(np.floor(np.quantile(vals, 0.05)))
            a, b = eng.links(m, t), eng.links(m, t + 0.75)
            assert_links(a, b, m)
            assert_links(a, expected(m, vals, n, n, True, t), m)
            for neg in (-0.5, -1e300, -INF):   # floor(T) < 0: nothing links (every count is >= 0)
                got = eng.links(m, neg)
                assert len(got[0]) == len(got[1]) == len(got[2]) == 0 and eng.last_links_calls == [], (m, neg)
                assert got[2].dtype == np.int64 and eng.links(m, neg, count_only=True) == 0
            got = eng.links(m, 1e300)   # clamped to the int64 range: everything links
            assert_links(got, expected(m, vals, n, n, True, INF), m)
            assert len(got[0]) == n * (n - 1) // 2


# ---- 7. tiny sets, errors ----------------------------------------------------------------------------------------------
def test_tiny_sets():
    codes = random_alignment(3, 50, seed=95, divergence=0.3)
    with da.Engine(0) as eng:
        with pytest.raises(da.DistanceError):
            eng.upload(0, codes[:0])   # (an empty set is not accepted by upload: n = 0 and an empty rectangle side cannot arise)
        eng.upload(0, codes[:1])
        got = eng.links("raw", INF, tallies=True)
        assert [len(x) for x in got] == [0, 0, 0, 0] and got[3].shape == (0, 2) and eng.last_links_calls == []
        assert eng.links("raw", INF, count_only=True) == 0
        eng.upload(0, np.ascontiguousarray(codes[[0, 0]]))
        got = eng.links("raw", 0.0)
        assert list(got[0]) == [0] and list(got[1]) == [1] and got[2][0] == 0.0 and eng.last_links_calls == [1]
        eng.upload(0, codes[:2])
        assert eng.run_square("n_high")[0] > 0
        assert len(eng.links("n_high", 0)[0]) == 0 and eng.last_links_calls == []
        eng.upload(1, codes[:1])   # a rectangle of 2 x 1 and 1 x 2
        for rs, cs in ((0, 1), (1, 0)):
            vals = eng.run_rect("raw", rs, cs)
            assert_links(eng.links("raw", INF, square=False, row_slot=rs, col_slot=cs),
                         expected("raw", vals, vals.shape[0], vals.shape[1], False, INF), (rs, cs))


def test_errors():
    lib = da.load()
    codes = random_alignment(50, 100, seed=96)
    calls = []
    sink = da.LINKS_SINK(lambda *a: calls.append(a[2]) or 0)
    total = C.c_uint64(7)

    def links(h, m=2, square=1, rs=0, cs=1, t=1.0, what=1, cb=sink):
        return lib.dst_links(h, m, square, rs, cs, t, 0, what, cb, None, C.byref(total))

    with da.Engine(0) as eng:
        h = eng._h
        assert links(h) == ERR_STATE and total.value == 0 and b"not uploaded" in lib.dst_last_error(h)
        eng.upload(0, codes)
        assert links(h, square=0) == ERR_STATE   # slot 1 is empty
        total.value = 7
        assert links(h, t=float("nan")) == ERR_ARG and total.value == 0
        assert links(h, m=9) == ERR_ARG and links(h, m=-1) == ERR_ARG
        assert links(h, what=4) == ERR_ARG and links(h, what=7) == ERR_ARG and links(h, what=4, cb=None) == ERR_ARG
        assert links(h, square=0, rs=2) == ERR_ARG and links(h, square=0, cs=-1) == ERR_ARG
        assert links(h, square=0, rs=1, cs=1) == ERR_ARG
        eng.upload(1, random_alignment(5, 90, seed=97))
        assert links(h, square=0) == ERR_STATE and b"Different length sequences" in lib.dst_last_error(h)
        assert calls == []
        assert links(h, t=INF) == 0 and total.value == 50 * 49 // 2 and calls == [50 * 49 // 2]
        assert lib.dst_links(h, 2, 1, 0, 1, INF, 0, 3, sink, None, None) == 0   # n_links may be NULL
        assert links(h, t=INF, what=3, cb=None) == 0 and total.value == 50 * 49 // 2 and len(calls) == 2   # count only


def test_sink_stops_the_run():
    lib = da.load()
    codes = random_alignment(60, 100, seed=98)
    seen = []

    def cb(_user, first, count, row, col, val, tal):
        seen.append((int(first), int(count), bool(val), bool(tal)))
        return 1 if len(seen) == 2 else 0

    sink = da.LINKS_SINK(cb)
    total = C.c_uint64()
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        before = eng.run_square("tn93")
        rc = lib.dst_links(eng._h, 2, 1, 0, 1, INF, 1, 1, sink, None, C.byref(total))   # one row per slab
        assert rc == ERR_STATE and b"stopped by sink" in lib.dst_last_error(eng._h)
        assert seen == [(0, 59, True, False), (59, 58, True, False)] and total.value == 59
        assert np.array_equal(bits(eng.run_square("tn93")), bits(before))   # the engine works on
        vals = eng.run_square("raw")
        assert_links(eng.links("raw", 0.05), expected("raw", vals, 60, 60, True, 0.05), "after the stop")


# ---- 8. the state a call leaves behind ---------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["auto", "dense", "consensus"])
def test_run_square_unchanged(sets, path):
    codes = sets["nrun"]
    n = len(codes)
    with da.Engine(0) as eng:
        eng.set_prep_threshold(0)
        eng.set_path(path)
        eng.upload(0, codes)
        for m in ("raw", "tn93"):
            before = eng.run_square(m)
            used = eng.last_path()
            t = interior(before)
            eng.links(m, t, max_pairs=2000, tallies=True)
            eng.links(m, t, count_only=True)
            after = eng.run_square(m)
            assert np.array_equal(bits(before), bits(after)) and eng.last_path() == used, (path, m)


def test_between_the_other_analyses(sets):
    """The slab scratch is shared: a tally walk and a payload walk of dst_links between the other analyses, each result
    that of a fresh context."""
    codes = sets["clade"]
    ops = (lambda e: e.nearest("tn93", k=3, tallies=True), lambda e: e.links("tn93", 0.002, max_pairs=500, tallies=True),
           lambda e: e.clusters("n_high", 3.0, max_pairs=500), lambda e: e.links("n_high", 3.0, max_pairs=700),
           lambda e: e.mst("raw", max_pairs=500), lambda e: e.links("raw", INF, count_only=True))
    fresh = []
    for op in ops:
        with da.Engine(0) as eng:
            eng.upload(0, codes)
            fresh.append(op(eng))

    def same(a, b):
        if isinstance(a, tuple):
            return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
        return np.array_equal(bits(a), bits(b)) if isinstance(a, np.ndarray) and a.dtype.itemsize == 8 else np.array_equal(a, b)

    with da.Engine(0) as eng:
        eng.upload(0, codes)
        for order in (range(len(ops)), reversed(range(len(ops)))):
            for k in order:
                assert same(ops[k](eng), fresh[k]), k


# ---- 9. full size ------------------------------------------------------------------------------------------------------
def test_full_size():
    """synth 10,000 x 30,000, -m n: T = 5 (on this alignment no pair is that close: the count is dst_clusters' all the
    same, and the sampled rows agree), and the 1 % quantile of row 0's values, at which row 0 alone holds ~100 links."""
    n, L = 10_000, 30_000
    codes = synth.alignment(synth.SEED, n, L)
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        rows = {r: eng.run_square("n", row_begin=r, row_end=r + 1) for r in (0, 4321, n - 2)}
        for t in (5, float(np.quantile(rows[0], 0.01))):
            row, col, val = eng.links("n", t)
            labels, n_links = eng.clusters("n", t)
            assert len(row) == n_links == eng.links("n", t, count_only=True), t
            assert np.all(row < col) and np.all(val <= t)
            key = row.astype(np.int64) * n + col
            assert np.all(np.diff(key) > 0)   # canonical order, no pair twice
            for r, v in rows.items():
                keep = v <= np.floor(t)
                mine = row == r
                assert np.array_equal(col[mine], (r + 1 + np.nonzero(keep)[0]).astype(np.uint32)), (t, r)
                assert np.array_equal(val[mine], v[keep]), (t, r)
        assert n_links >= 50   # (the second threshold links pairs: row 0's share alone)
