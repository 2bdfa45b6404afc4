"""GPU (-m gpu): run_windows, nearest_windows, run_pairs and the window-closest stream on the designed sets of
record_boundary_cases.py.  The 92,700 records (record indices of 17 bits, canonical ordinals of 33) put window rows, pair
lists and candidate lists on both sides of record 65,536 and of offset 2^32; the tall set of 524,289 records gives one
window launch more than 65,535 row tiles, a second launch grid.  n, raw and the tallies are compared bit for bit with the
windowed closed forms (test_record_boundary_host.py holds those to the oracle, and the sizes below to what they claim);
tn93, jc69 and k80 with the oracle at the suite's 1e-12 bar, or bitwise with run_square / run_rect on the set cut to the
window, the contract dst_run_windows documents."""
import functools

import numpy as np
import pytest

import distance_amd as da
import oracle
import record_boundary_cases as rbc
from closest_reference import keys, smallest
from record_boundary_cases import FIRST_ROW_PAST_2_32, NEAREST_WINDOWS, POP, WINDOWS
from test_gpu_parity import assert_close
from window_reference import pair_index

pytestmark = pytest.mark.gpu
THREADS = 16
DEFAULT_MAX_PAIRS = 1 << 25        # the slab bound of an analysis that is given none
TALL_WINDOWS = ((0, 40), (3, 17))
LOG_MEASURES = ("tn93", "jc69", "k80")


@pytest.fixture(scope="module")
def rs():
    return rbc.record_set()


@pytest.fixture(scope="module")
def eng(rs):
    e = da.Engine(0)
    e.upload(0, rs.codes)
    e.in_slot_1 = None
    yield e
    e.close()


def fill_slot_1(eng, rs, what):
    """slot 1 holds the picked records ("picked") or all 92,700 again ("all"): uploaded when it holds the other"""
    if eng.in_slot_1 != what:
        eng.upload(1, np.ascontiguousarray(rs.codes[rs.picked]) if what == "picked" else rs.codes)
        eng.in_slot_1 = what


@pytest.fixture(scope="module")
def tall():
    return rbc.tall_set()


@pytest.fixture(scope="module")
def tall_eng(tall):
    """slot 0 the tall set, slot 1 five of its records"""
    e = da.Engine(0)
    e.upload(0, tall.codes)
    e.upload(1, np.ascontiguousarray(tall.codes[rbc.tall_columns()]))
    yield e
    e.close()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same_bits(got, want):
    """equal shapes, types and bits; for f64 a NaN of the closed form (0 / 0, whose sign numpy does not promise) matches any
    NaN"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype != np.float64:
        return np.array_equal(got, want)
    return bool(((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all())


def same_bits_exactly(got, want):
    """two results of the engine: every bit, NaN included"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    return np.array_equal(bits(got), bits(want))


def cut(codes, b, e):
    return np.ascontiguousarray(codes[:, b:e])


def assert_windows(rs, got_of, i, j, windows=WINDOWS, values=("n", "raw"), tallies=("raw", "k80", "tn93")):
    """got_of(measure, tallies) = run_windows' (n_windows, P[, width]) of the pairs (i, j) against the closed forms"""
    for m in values:
        got = got_of(m, False)
        assert got.shape == (len(windows), len(i))
        for w, (b, e) in enumerate(windows):
            assert same_bits(got[w], rs.window_values(m, i, j, b, e)), (m, b, e)
    for m in tallies:
        got = got_of(m, True)
        for w, (b, e) in enumerate(windows):
            assert same_bits(got[w], rs.window_tallies(m, i, j, b, e).astype(np.uint32)), (m, b, e)


# ---- a. run_windows, square ----------------------------------------------------------------------------------------------
SQUARE_ROWS = [(65_534, 65_538), (FIRST_ROW_PAST_2_32 - 2, FIRST_ROW_PAST_2_32 + 3), (rbc.N_RECORDS - 3, rbc.N_RECORDS)]


@pytest.mark.parametrize("rows", SQUARE_ROWS)
def test_run_windows_square(eng, rs, rows):
    """rows either side of record 65,536 (tri_row_start and i of 17 bits, 363 column tiles), either side of the first row
    whose start is at or above 2^32 (out_base and tri_row_start of 33 bits), and the last rows"""
    rb, re = rows
    i, j = pair_index(True, rs.n, rs.n, rb, re)
    assert len(i) == rbc.row_start(rs.n, re) - rbc.row_start(rs.n, rb)
    assert_windows(rs, lambda m, t: eng.run_windows(m, WINDOWS, row_begin=rb, row_end=re, tallies=t), i, j)


def test_run_windows_square_is_run_square_of_the_cut_set(eng, rs):
    """tn93 of the rows around the 2^32 offset: bitwise the second engine's run_square on codes[:, b:e], NaN included, and
    with jc69 and k80 within 1e-12 of the oracle on the same columns"""
    rb, re = SQUARE_ROWS[1]
    i, j = pair_index(True, rs.n, rs.n, rb, re)
    got = {m: eng.run_windows(m, WINDOWS, row_begin=rb, row_end=re) for m in LOG_MEASURES}
    with da.Engine(0) as other:
        for w, (b, e) in enumerate(WINDOWS):
            if e <= b:
                continue
            codes = cut(rs.codes, b, e)
            other.upload(0, codes)
            assert same_bits_exactly(got["tn93"][w], other.run_square("tn93", rb, re)), (b, e)
            counts = rs.window_base_counts(b, e).astype(np.uint64)
            for m in LOG_MEASURES:
                full = oracle.all_pairs_rect(m, codes[rb:re], codes, counts[rb:re], counts, threads=THREADS).reshape(re - rb, rs.n)
                assert_close(got[m][w], full[i - rb, j])


def test_window_base_counts(eng, rs):
    got = eng.window_base_counts(0, WINDOWS)
    assert got.shape == (len(WINDOWS), rs.n, 4)
    for w, (b, e) in enumerate(WINDOWS):
        assert same_bits(got[w], rs.window_base_counts(b, e)), (b, e)


# ---- b. run_windows, rectangles ------------------------------------------------------------------------------------------
def test_run_windows_rect_picked_rows_by_all_columns(eng, rs):
    """ten picked records, among them 65,534 .. 65,537, against all 92,700 columns: 363 column tiles (the tile count is the
    columns'; all 300 picked rows x 7 windows would be 3 GB of tn93 tallies)"""
    fill_slot_1(eng, rs, "picked")
    assert -(-rs.n // 256) == 363
    p0 = int(np.searchsorted(rs.picked, 65_534)) - 3
    rows = rs.picked[p0:p0 + 10]
    assert {65_534, 65_535, 65_536, 65_537} <= set(rows.tolist())
    i, j = [x.ravel() for x in np.meshgrid(rows, np.arange(rs.n), indexing="ij")]
    kw = dict(square=False, row_slot=1, col_slot=0, row_begin=p0, row_end=p0 + 10)
    assert_windows(rs, lambda m, t: eng.run_windows(m, WINDOWS, tallies=t, **kw), i, j)
    got = eng.run_windows("tn93", WINDOWS, **kw)
    with da.Engine(0) as other:
        for w, (b, e) in enumerate(WINDOWS):
            if e > b:
                other.upload(0, cut(rs.codes, b, e))
                other.upload(1, cut(rs.codes[rs.picked], b, e))
                assert same_bits_exactly(got[w], other.run_rect("tn93", 1, 0, p0, p0 + 10).ravel()), (b, e)


def test_run_windows_rect_rows_past_65535_by_picked_columns(eng, rs):
    """rows [65,530, 65,540) of the set against the picked records: i - row_begin and i of 17 bits in the rectangle's address"""
    fill_slot_1(eng, rs, "picked")
    rb, re = 65_530, 65_540
    i, j = [x.ravel() for x in np.meshgrid(np.arange(rb, re), rs.picked, indexing="ij")]
    kw = dict(square=False, row_slot=0, col_slot=1, row_begin=rb, row_end=re)
    assert_windows(rs, lambda m, t: eng.run_windows(m, WINDOWS, tallies=t, **kw), i, j)
    got = {m: eng.run_windows(m, WINDOWS, **kw) for m in LOG_MEASURES}
    for w, (b, e) in enumerate(WINDOWS):
        if e > b:
            codes, counts = cut(rs.codes, b, e), rs.window_base_counts(b, e).astype(np.uint64)
            for m in LOG_MEASURES:
                want = oracle.all_pairs_rect(m, codes[rb:re], codes[rs.picked], counts[rb:re], counts[rs.picked], threads=THREADS)
                assert_close(got[m][w], want.ravel())


# ---- c. run_pairs --------------------------------------------------------------------------------------------------------
def slab_bound(rs, cut_at):
    if cut_at == "default":
        return DEFAULT_MAX_PAIRS
    if cut_at == "row_65536":
        return rbc.max_pairs_cutting_in(rs.n, 65_536, 65_536)
    return rbc.max_pairs_cutting_in(rs.n, FIRST_ROW_PAST_2_32, rs.n - 2)


def assert_pairs(eng, rs, row, col, route, **kw):
    """both outputs together and each alone, against the closed forms (which have the diagonal at 0); the info of the run
    with both outputs"""
    for m in ("n", "raw", "k80", "tn93"):
        want_t = rs.tallies(m, row, col).astype(np.uint32)
        got_v, got_t, info = eng.run_pairs(m, row, col, values=True, tallies=True, route=route, info=True, **kw)
        assert same_bits(got_t, want_t), (m, route, "tallies")
        assert same_bits(eng.run_pairs(m, row, col, values=False, tallies=True, route=route, **kw), want_t), (m, route, "tallies alone")
        alone = eng.run_pairs(m, row, col, route=route, **kw)
        assert same_bits_exactly(alone, got_v), (m, route, "values alone")
        if m in ("n", "raw"):
            assert same_bits(got_v, rs.values(m, row, col)), (m, route, "values")
    return info


@pytest.mark.parametrize("cut_at", ["default", "row_65536", "past_2_32"])
def test_run_pairs_sweep(eng, rs, cut_at):
    """canonical positions, slab starts and pos = position - first of 33 bits; a slab boundary at row 65,536; a slab that
    begins at or above 2^32"""
    row, col = rbc.boundary_pairs()
    bound = slab_bound(rs, cut_at)
    info = assert_pairs(eng, rs, row, col, "sweep", max_pairs=0 if cut_at == "default" else bound)
    diagonal = int((row == col).sum())
    assert info["route"] == "sweep" and info["slabs"] == len(rbc.touched_slabs(rs.n, bound, row, col))
    assert info["direct_pairs"] == diagonal == 4 and info["swept_pairs"] == len(row) - diagonal


def test_run_pairs_direct(eng, rs):
    """the gather of record indices up to 92,699"""
    row, col = rbc.boundary_pairs()
    info = assert_pairs(eng, rs, row, col, "direct")
    assert info["route"] == "direct" and info["direct_pairs"] == len(row) and info["slabs"] == 0


@pytest.mark.parametrize("route", ["direct", "sweep"])
def test_run_pairs_rect(eng, rs, route):
    """92,700 x 92,700: positions i n + j either side of 2^32"""
    fill_slot_1(eng, rs, "all")
    row, col = rbc.boundary_rect_pairs()
    info = assert_pairs(eng, rs, row, col, route, square=False, row_slot=0, col_slot=1)
    assert info["route"] == route and (info["direct_pairs"], info["swept_pairs"]) == ((len(row), 0) if route == "direct" else (0, len(row)))


@pytest.mark.parametrize("measure", LOG_MEASURES)
def test_run_pairs_log_measures(eng, rs, measure):
    """the two routes agree bitwise, at every slab bound, and lie within 1e-12 of the oracle's value of the two records"""
    fill_slot_1(eng, rs, "all")
    counts = rs.base_counts().astype(np.uint64)
    for square, (row, col) in ((True, rbc.boundary_pairs()), (False, rbc.boundary_rect_pairs())):
        kw = {} if square else dict(square=False, row_slot=0, col_slot=1)
        direct = eng.run_pairs(measure, row, col, route="direct", **kw)
        for cut_at in ("default", "row_65536", "past_2_32") if square else ("default",):
            swept = eng.run_pairs(measure, row, col, route="sweep", max_pairs=slab_bound(rs, cut_at), **kw)
            assert same_bits_exactly(swept, direct), (square, cut_at)
        lo, hi = (np.minimum(row, col), np.maximum(row, col)) if square else (row, col)
        want = np.array([oracle.pair_distance(measure, rs.codes[a], rs.codes[b], counts[a], counts[b])
                         for a, b in zip(lo.tolist(), hi.tolist())])
        assert_close(direct, want)


# ---- d. more than 524,280 rows in one window launch ----------------------------------------------------------------------
def tall_pairs(tall, row_begin=0):
    i = np.repeat(np.arange(row_begin, tall.n), 5)
    j = np.tile(rbc.tall_columns(), tall.n - row_begin)
    return i, j


@pytest.mark.parametrize("row_begin", [0, rbc.TALL_ROW_BEGIN])
def test_tall_run_windows(tall_eng, tall, row_begin):
    """65,537 row tiles: the second grid's rows 524,280 .. 524,288 (row begin 3: 524,283 .., off a multiple of 8); every row
    is compared"""
    assert rbc.second_grid_first_row(row_begin, tall.n) == 524_280 + row_begin
    i, j = tall_pairs(tall, row_begin)
    kw = dict(square=False, row_slot=0, col_slot=1, row_begin=row_begin)
    assert_windows(tall, lambda m, t: tall_eng.run_windows(m, TALL_WINDOWS, tallies=t, **kw), i, j, windows=TALL_WINDOWS,
                   values=("n",), tallies=("tn93",))


def ascending(key_rows, k):
    """positions of the k smallest (key, position) of every row: closest_reference.smallest, all rows at once (a stable
    sort leaves equal keys in position order), and held to it on a few rows"""
    pos = np.argsort(key_rows, axis=1, kind="stable")[:, :k]
    for r in (0, 1, len(key_rows) // 2, len(key_rows) - 1):
        assert np.array_equal(pos[r], smallest(np.ascontiguousarray(key_rows[r]), k))
    return pos


@functools.lru_cache(maxsize=None)
def tall_selection(measure, windows, k=2):
    """(index, values or None, tallies) [524,289][windows][k]: every tall record's k nearest of the five column records"""
    tall, cols = rbc.tall_set(), rbc.tall_columns()
    rows = np.arange(tall.n)
    index, values, tallies = [], [], []
    for b, e in windows:
        if measure == "tn93":   # the set holds no T: the oracle's value is NaN for every pair, so the order is the index's
            codes, counts = cut(tall.codes, b, e), tall.window_base_counts(b, e).astype(np.uint64)
            vals = oracle.all_pairs_rect("tn93", codes, codes[cols], counts, counts[cols], threads=THREADS).reshape(tall.n, 5)
            assert np.isnan(vals).all()
        else:
            vals = np.stack([tall.window_values(measure, rows, np.full(tall.n, c), b, e) for c in cols], axis=1)
        pos = ascending(keys(vals).reshape(tall.n, 5), k)
        index.append(pos)
        values.append(np.take_along_axis(vals, pos, axis=1))
        tallies.append(tall.window_tallies(measure, np.repeat(rows, k), cols[pos].ravel(), b, e).reshape(tall.n, k, -1))
    return (np.stack(index, axis=1).astype(np.uint32), np.stack(values, axis=1), np.stack(tallies, axis=1).astype(np.uint32))


def assert_selection(got, want, measure):
    """(index, values, tallies): index and tallies bit for bit; n's values too, tn93's within the bar of the oracle's"""
    assert same_bits(got[0], want[0]), (measure, "index")
    if measure == "tn93":
        assert_close(got[1], want[1])
    else:
        assert same_bits(got[1], want[1]), (measure, "values")
    assert same_bits(got[2], want[2]), (measure, "tallies")


@pytest.mark.parametrize("n_windows", [1, 2])
@pytest.mark.parametrize("measure", ["n", "tn93"])
def test_tall_nearest_windows(tall_eng, tall, measure, n_windows):
    """one slab of all 524,289 rows (the default max_entries): the sweep's second grid, and lists of rows past 524,280"""
    windows = TALL_WINDOWS[:n_windows]
    assert rbc.cut_window_slabs(tall.n, n_windows, 5) == (tall.n, n_windows)
    got = tall_eng.nearest_windows(measure, windows, 2, square=False, row_slot=0, col_slot=1, tallies=True)
    assert_selection(got, tall_selection(measure, windows), measure)


@pytest.mark.parametrize("measure", ["n", "tn93"])
def test_tall_window_closest_stream(tall_eng, tall, measure):
    """the tall set loaded, one batch of the five records: the stream sweeps all 524,289 loaded records as rows of one range"""
    cols = rbc.tall_columns()
    with tall_eng.window_closest_stream(measure, TALL_WINDOWS, 2, max_records=5, depth=2) as st:
        st.push(tall.codes[cols])
        assert st.pop() == 5
        got = st.result(tallies=True, counts=measure == "tn93")
    want = tall_selection(measure, TALL_WINDOWS)
    assert_selection(got, want, measure)
    if measure == "tn93":
        for w, (b, e) in enumerate(TALL_WINDOWS):
            assert same_bits(got[3][:, w], tall.window_base_counts(b, e)[cols[want[0][:, w].astype(np.int64)]]), (b, e)


# ---- e. nearest_windows on the 92,700 records ----------------------------------------------------------------------------
def window_selection(rs, measure, rows, windows, k, exclude_self):
    """(index, values, tallies) [rows][windows][k] by brute force over whole rows of the closed form: ascending (key, index),
    the row's own record no candidate when exclude_self"""
    everyone = np.arange(rs.n)
    index = np.zeros((len(rows), len(windows), k), np.uint32)
    for a, r in enumerate(rows):
        cand = np.delete(everyone, r) if exclude_self else everyone
        for w, (b, e) in enumerate(windows):
            vals = rs.window_values(measure, np.full(len(cand), r), cand, b, e)
            index[a, w] = cand[smallest(keys(vals), k)]
    i = np.repeat(np.asarray(rows, np.int64), len(windows) * k)
    shape = (len(rows), len(windows), k)
    values = np.zeros(shape, np.int64 if measure == "n" else np.float64)
    tallies = np.zeros(shape + (1 if measure == "n" else 2,), np.uint32)
    for w, (b, e) in enumerate(windows):
        ii, jj = np.repeat(np.asarray(rows, np.int64), k), index[:, w].astype(np.int64).ravel()
        values[:, w] = rs.window_values(measure, ii, jj, b, e).reshape(len(rows), k)
        tallies[:, w] = rs.window_tallies(measure, ii, jj, b, e).reshape(len(rows), k, -1)
    return index, values, tallies


@pytest.mark.parametrize("rows", [(65_530, 65_540), (rbc.N_RECORDS - 10, rbc.N_RECORDS)])
def test_nearest_windows_square(eng, rs, rows):
    """rows past 65,535 with candidates on both sides of them: i = row0 + il excluded, lists at (i n_windows + w) k.  The
    window (38, 40) is almost all ties, which resolve by index; its raw is NaN wherever a record has both sites N"""
    rb, re = rows
    cases = [("n", 8), ("raw", 8)] + ([("n", 256)] if rb == 65_530 else [])
    for measure, k in cases:
        kw = dict(row_begin=rb, row_end=re, tallies=True)
        got = eng.nearest_windows(measure, NEAREST_WINDOWS, k, **kw)
        assert got[0].shape == (re - rb, len(NEAREST_WINDOWS), k)
        for max_entries in (1, rs.n * 16):   # every slab one (row, window); a few rows x all windows
            other = eng.nearest_windows(measure, NEAREST_WINDOWS, k, max_entries=max_entries, **kw)
            assert all(same_bits_exactly(g, o) for g, o in zip(got, other)), (measure, k, max_entries)
        assert_selection(got, window_selection(rs, measure, range(rb, re), NEAREST_WINDOWS, k, True), measure)
        own = np.arange(rb, re, dtype=np.uint32)[:, None, None]
        assert not (got[0] == own).any()
        if measure == "n":   # no varying site in (38, 40): every candidate at 0, the first k records in index order
            ties = NEAREST_WINDOWS.index((38, 40))
            assert not got[1][:, ties].any() and (got[0][:, ties] == np.arange(k, dtype=np.uint32)).all()


@pytest.mark.parametrize("measure", ["n", "raw"])
def test_nearest_windows_rect(eng, rs, measure):
    """the picked records against all 92,700: candidates j up to 92,699, itself first at 0"""
    fill_slot_1(eng, rs, "picked")
    got = eng.nearest_windows(measure, NEAREST_WINDOWS, 8, square=False, row_slot=1, col_slot=0, tallies=True)
    assert_selection(got, window_selection(rs, measure, rs.picked, NEAREST_WINDOWS, 8, False), measure)
    assert (got[0] >= 65_536).any() and np.array_equal(got[0][:, 0, 0], rs.picked.astype(np.uint32))


# ---- f. the window-closest stream on the 92,700 records ------------------------------------------------------------------
def stream_reference(rs, measure, streamed, windows, k):
    """index [loaded][windows][k]: per (loaded record, window) the k smallest (key, ordinal) over the streamed records, by
    brute force with POP over 92,700 x 300 per window.  The values of n and raw are d / comparable with d <= 20 and three
    denominators, so the keys' order is a table rank[d][max residue]; tn93 is NaN for every pair (the set holds no T)."""
    n, worst = rs.n, np.maximum((np.arange(rs.n) % 3).astype(np.int8)[:, None], (streamed % 3).astype(np.int8)[None, :])
    ordinal = np.arange(len(streamed), dtype=np.int32)[None, :]
    assert len(streamed) <= 512
    index = np.zeros((n, len(windows), k), np.uint32)
    for w, (b, e) in enumerate(windows):
        if measure == "tn93":
            codes, counts = cut(rs.codes, b, e), rs.window_base_counts(b, e).astype(np.uint64)
            vals = oracle.all_pairs_rect("tn93", codes[streamed], codes, counts[streamed], counts, threads=THREADS)
            assert np.isnan(vals).all()
            index[:, w] = np.arange(k, dtype=np.uint32)
            continue
        d = POP[(rs.words[:, None] ^ rs.words[streamed][None, :]) & rbc.window_mask(b, e)]
        dd, ww = [x.ravel() for x in np.meshgrid(np.arange(rbc.BITS + 1), np.arange(3), indexing="ij")]
        comp = rs.window_comparable(ww, np.zeros(3 * (rbc.BITS + 1), np.int64), b, e)   # (record 0 has no N: the other's count)
        with np.errstate(invalid="ignore", divide="ignore"):
            table = dd.astype(np.int64) if measure == "n" else dd.astype(np.float64) / comp.astype(np.float64)
        rank = np.unique(keys(table), return_inverse=True)[1].reshape(rbc.BITS + 1, 3).astype(np.int32)
        combined = rank[d, worst] * 512 + ordinal
        index[:, w] = np.sort(np.partition(combined, k - 1, axis=1)[:, :k], axis=1) & 511
    return index


@pytest.mark.parametrize("measure", ["n", "raw", "tn93"])
def test_window_closest_stream(eng, rs, measure):
    """the 300 picked records streamed in batches of 128, 128 and 44 past the loaded 92,700: lists of loaded records past
    65,535, ordinals across the batches"""
    streamed, k = rs.picked, 4
    with eng.window_closest_stream(measure, NEAREST_WINDOWS, k, max_records=128, depth=2) as st:
        for b0 in range(0, len(streamed), 128):
            st.push(rs.codes[streamed[b0:b0 + 128]])
            assert st.pop() == min(128, len(streamed) - b0)
        got = st.result(tallies=True, counts=measure == "tn93")
    assert len(streamed) % 128 != 0 and got[0].shape == (rs.n, len(NEAREST_WINDOWS), k)
    index = stream_reference(rs, measure, streamed, NEAREST_WINDOWS, k)
    assert same_bits(got[0], index)
    loaded = np.repeat(np.arange(rs.n), k)
    for w, (b, e) in enumerate(NEAREST_WINDOWS):
        partner = streamed[index[:, w].astype(np.int64)].ravel()
        assert same_bits(got[2][:, w].reshape(len(loaded), -1), rs.window_tallies(measure, loaded, partner, b, e).astype(np.uint32)), (b, e)
        if measure == "tn93":
            assert np.isnan(got[1][:, w]).all(), (b, e)
            assert same_bits(got[3][:, w].reshape(len(loaded), 4), rs.window_base_counts(b, e)[partner]), (b, e)
        else:
            assert same_bits(got[1][:, w].ravel(), rs.window_values(measure, loaded, partner, b, e)), (b, e)
