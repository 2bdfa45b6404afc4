"""GPU (-m gpu): every slab-driven analysis on the designed set of record_boundary_cases.py: 92,700 records, 4,296,598,650
pairs.  Record indices need 17 bits, canonical ordinals 33, the default cut's last slab straddles offset 2^32, and chosen
slab bounds put a cut at row 65,536, begin a slab at or above 2^32 and make one slab of more than 65,535 rows (a second
launch grid).  Every answer is compared with the set's closed forms (test_record_boundary_host.py holds those to the
oracle) or with the oracle itself: n, raw and tallies bit for bit, tn93 and jc69 at the suite's 1e-12 bar on picked pairs."""
import ctypes as C
import functools

import numpy as np
import pytest

import distance_amd as da
import oracle
import pair_sites_reference
import record_boundary_cases as rbc
import summary_reference
from closest_reference import keys, smallest
from mst_reference import components
from record_boundary_cases import FIRST_ROW_PAST_2_32, POP, TWO32, canon
from test_gpu_parity import assert_close

pytestmark = pytest.mark.gpu
THREADS = 16
RAW_T1, RAW_T2 = 0.04, 0.0505   # 1/38 < RAW_T1 < 2/40 < RAW_T2 < 2/39


@pytest.fixture(scope="module")
def rs():
    return rbc.record_set()


@pytest.fixture(scope="module")
def eng(rs):
    e = da.Engine(0)
    e.upload(0, rs.codes)
    e.set_ids(0, rs.ids())
    yield e
    e.close()


@pytest.fixture(scope="module")
def picked_slot(eng, rs):
    """the picked records as slot 1, with their ids"""
    eng.upload(1, np.ascontiguousarray(rs.codes[rs.picked]))
    ids = rs.ids()
    eng.set_ids(1, [ids[r] for r in rs.picked])
    return rs.picked


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    return np.array_equal(got.view(np.uint64) if got.dtype == np.float64 else got, want.view(np.uint64) if want.dtype == np.float64 else want)


# ---- a. the anchor: the pair kernels and the closed forms agree on this set ---------------------------------------------
def test_run_square_of_the_picked_rows(eng, rs):
    n = rs.n
    cols_all = np.arange(n)
    for r in rs.picked[rs.picked < n - 1]:
        r = int(r)
        cols = cols_all[r + 1:]
        rows = np.full(len(cols), r)
        assert same_bits(eng.run_square("n", r, r + 1), rs.values("n", rows, cols)), r
        assert same_bits(eng.run_square("n_high", r, r + 1), rs.values("n_high", rows, cols)), r
        assert same_bits(eng.run_square("raw", r, r + 1), rs.values("raw", rows, cols)), r
        assert same_bits(eng.run_square("tn93", r, r + 1, tallies=True), rs.tallies("tn93", rows, cols).astype(np.uint32)), r
    assert same_bits(eng.base_counts(0), rs.base_counts())


@pytest.mark.parametrize("measure", ["tn93", "jc69", "k80"])
def test_run_square_log_measures_against_the_oracle(eng, rs, measure):
    """(tn93 is NaN for every pair of this set, which holds no T: its check is the NaN pattern, and its tallies above)"""
    counts = rs.base_counts().astype(np.uint64)
    for r in rbc.FIXED_ROWS[:-1]:
        want = oracle.all_pairs_rect(measure, rs.codes[r:r + 1], rs.codes[r + 1:], counts[r:r + 1], counts[r + 1:],
                                     threads=THREADS)[0]
        assert_close(eng.run_square(measure, r, r + 1), want)


# ---- b. links ---------------------------------------------------------------------------------------------------------------
def assert_links(rs, got, measure, keep_of):
    """got = Engine.links(..., tallies=True) against the reference list restricted by keep_of(i, j, d)"""
    i, j, d = rs.links_within(2)
    keep = keep_of(i, j, d)
    i, j = i[keep], j[keep]
    assert same_bits(got[0], i.astype(np.uint32)) and same_bits(got[1], j.astype(np.uint32))
    assert same_bits(got[2], rs.values(measure, i, j))
    assert same_bits(got[3], rs.tallies(measure, i, j).astype(np.uint32))
    return len(i)


@pytest.mark.parametrize("measure", ["n", "n_high"])
@pytest.mark.parametrize("T", [1, 2])
def test_links_n(eng, rs, measure, T):
    got = eng.links(measure, T, tallies=True)
    count = assert_links(rs, got, measure, lambda i, j, d: d <= T)
    assert count == (81_846, 860_980)[T - 1]
    at = canon(rs.n, got[0], got[1])
    assert (at >= TWO32).sum() == (30, 346)[T - 1] and (got[0] >= 65_536).any() and (got[1] >= 65_536).any()


@pytest.mark.parametrize("path", ["dense", "consensus"])
def test_links_count_only_on_both_paths(eng, rs, path):
    eng.set_path(path)
    try:
        assert eng.links("n", 2, count_only=True) == 860_980
        assert eng.last_path() == path
    finally:
        eng.set_path("auto")


@pytest.mark.parametrize("cut", ["row_65536", "past_2_32"])
def test_links_slab_bounds(eng, rs, cut):
    """a slab boundary at row 65,535 | 65,536; a last slab whose out_base is at or above 2^32"""
    n = rs.n
    bound = rbc.max_pairs_cutting_in(n, 65_536, 65_536) if cut == "row_65536" else rbc.max_pairs_cutting_in(n, FIRST_ROW_PAST_2_32, n - 2)
    got = eng.links("n", 2, max_pairs=bound, tallies=True)
    assert assert_links(rs, got, "n", lambda i, j, d: d <= 2) == 860_980


@pytest.mark.parametrize("T", [RAW_T1, RAW_T2])
def test_links_raw_orders_by_value_not_by_count(eng, rs, T):
    """RAW_T1 links exactly the distance-1 pairs; RAW_T2 adds the distance-2 pairs of two records with all 40 sites"""
    got = eng.links("raw", T, tallies=True)
    if T == RAW_T1:
        count = assert_links(rs, got, "raw", lambda i, j, d: d == 1)
        assert count == 81_846
    else:
        count = assert_links(rs, got, "raw", lambda i, j, d: (d == 1) | (rs.comparable(i, j) == 40))
        assert 81_846 < count < 860_980


# ---- c. clusters ------------------------------------------------------------------------------------------------------------
def test_clusters(eng, rs):
    labels, links = eng.clusters("n", 1)
    assert links == 81_846 and same_bits(labels, rs.clusters(1))
    labels, links = eng.clusters("n", 0)
    assert links == 0 and same_bits(labels, np.arange(rs.n, dtype=np.uint32))


# ---- d. summary -------------------------------------------------------------------------------------------------------------
def square_summary_reference(rs):
    i, j, d = rs.links_within(1)
    hist = np.zeros(32, np.uint64)
    hist[:rbc.BITS + 1] = rs.histogram()
    pairs = rs.n * (rs.n - 1) // 2
    return {"within": rs.within(i, j), "summable": np.full(rs.n, rs.n - 1, np.uint32), "sum": rs.sums().astype(np.float64),
            "hist": hist, "pairs": pairs, "nan_pairs": 0, "summable_pairs": pairs, "links": len(i),
            "total_sum": float(int(rs.sums().sum()) // 2)}


def test_summary_square(eng, rs):
    got = eng.summary("n", 1, bins=32, width=1)
    summary_reference.assert_summary(got, square_summary_reference(rs), "square")


@functools.lru_cache(maxsize=None)
def picked_rect_values(measure):
    """the oracle's values of the picked records against the whole set"""
    rs = rbc.record_set()
    counts = rs.base_counts().astype(np.uint64)
    return oracle.all_pairs_rect(measure, rs.codes[rs.picked], rs.codes, counts[rs.picked], counts, threads=THREADS)


def test_summary_rect_raw(eng, rs, picked_slot):
    vals = picked_rect_values("raw")
    want = summary_reference.summary("raw", vals, len(picked_slot), rs.n, False, RAW_T2, bins=24, width=0.025)
    got = eng.summary("raw", RAW_T2, square=False, row_slot=1, col_slot=0, bins=24, width=0.025)
    summary_reference.assert_summary(got, want, "rect raw")
    assert int(want["within"].min()) >= 1   # (every picked record meets itself at 0)


def test_summary_rect_tn93(eng, rs, picked_slot):
    """the set holds no T, so tn93's k2 is 0 and the oracle's value of every pair is NaN: the summary has nothing to sum"""
    vals = picked_rect_values("tn93")
    assert np.isnan(vals).all()
    want = summary_reference.summary("tn93", vals, len(picked_slot), rs.n, False, 0.05, bins=24, width=0.025)
    got = eng.summary("tn93", 0.05, square=False, row_slot=1, col_slot=0, bins=24, width=0.025)
    summary_reference.assert_summary(got, want, "rect tn93")
    assert got["nan_pairs"] == len(picked_slot) * rs.n


def test_summary_rect_jc69(eng, rs, picked_slot):
    """a measure with a logarithm and finite values here.  jc69 is held to the oracle at 1e-12, so the threshold and the
    bin edges lie where no oracle value comes within 1e-9 of them: then the integers are exact, and a sum of 92,700 values
    may differ by 92,700 (1e-12 + 2^-38), the bar plus half a unit of the fixed point of the sums"""
    vals = picked_rect_values("jc69")
    T, width, bins = 0.0777, 0.0333, 24
    distinct = np.unique(vals)
    assert np.isfinite(distinct).all() and len(distinct) < 100
    assert all(np.abs(distinct - e).min() > 1e-9 for e in [T] + [width * b for b in range(1, bins)])
    want = summary_reference.summary("jc69", vals, len(picked_slot), rs.n, False, T, bins=bins, width=width)
    got = eng.summary("jc69", T, square=False, row_slot=1, col_slot=0, bins=bins, width=width)
    for key in ("pairs", "nan_pairs", "summable_pairs", "links"):
        assert got[key] == want[key], key
    for key in ("within", "summable", "hist"):
        assert np.array_equal(got[key], want[key]), key
    tol = rs.n * (1e-12 + 2.0 ** -38)
    assert np.abs(got["sum"] - want["sum"]).max() <= tol
    assert abs(got["total_sum"] - want["total_sum"]) <= tol * len(picked_slot)


# ---- e. nearest -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def nearest_reference(measure, exclude_self):
    """(index, values) [picked][256] by brute force over whole rows: ascending (value, index)"""
    rs = rbc.record_set()
    index, values = [], []
    for r in rs.picked:
        vals = rs.row(measure, int(r))
        k = keys(vals)
        if exclude_self:
            k[r] = np.uint64(0xFFFFFFFFFFFFFFFF)
        pos = smallest(k, 256)
        index.append(pos)
        values.append(vals[pos])
    return np.array(index, np.uint32), np.array(values)


@pytest.mark.parametrize("measure", ["n", "raw"])
@pytest.mark.parametrize("k", [8, 256])
def test_nearest_square(eng, rs, measure, k):
    index, values = eng.nearest(measure, k)
    want_index, want_values = nearest_reference(measure, True)
    assert same_bits(index[rs.picked], want_index[:, :k]) and same_bits(values[rs.picked], want_values[:, :k])
    if measure == "n" and k == 8:
        assert (want_values[:, 7] == 2).sum() >= len(rs.picked) - 3   # lists full of ties at K = 8
        # every row: the first neighbour is at 1 exactly where the record has a distance-1 link, and is its smallest partner
        i, j, _ = rs.links_within(1)
        first = np.full(rs.n, rs.n, np.int64)
        np.minimum.at(first, i, j)
        np.minimum.at(first, j, i)
        has = first < rs.n
        assert np.array_equal(values[:, 0] == 1, has) and (values[:, 0] >= 1).all()
        assert np.array_equal(index[has, 0], first[has].astype(np.uint32))


@pytest.mark.parametrize("measure", ["n", "raw"])
def test_nearest_rect(eng, rs, picked_slot, measure):
    index, values = eng.nearest(measure, 8, square=False, row_slot=1, col_slot=0)
    want_index, want_values = nearest_reference(measure, False)
    assert same_bits(index, want_index[:, :8]) and same_bits(values, want_values[:, :8])
    assert np.array_equal(index[:, 0], picked_slot.astype(np.uint32))   # itself, at 0


# ---- f. mst -----------------------------------------------------------------------------------------------------------------
def test_mst(eng, rs):
    edges, values, rounds = eng.mst("n")
    want_edges, want_values, _ = rs.mst()
    assert len(edges) == rs.n - 1 and 1 <= rounds <= 17
    assert same_bits(edges, want_edges.astype(np.uint32)) and same_bits(values, want_values)
    near = values <= 1
    assert same_bits(components(rs.n, edges[near, 0], edges[near, 1]), rs.clusters(1))


# ---- g. pair_sites ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", ["n", "tn93"])
def test_pair_sites(eng, rs, measure):
    rng = np.random.default_rng(11)
    fixed = np.array(rbc.FIXED_ROWS)
    row = np.concatenate([rng.integers(0, rs.n, 5_000), np.repeat(fixed, len(fixed)), fixed[:3], fixed[:3]])
    col = np.concatenate([rng.integers(0, rs.n, 5_000), np.tile(fixed, len(fixed)), fixed[-3:], fixed[-3:]])
    offsets, sites, bases = eng.pair_sites(measure, row, col)
    want = pair_sites_reference.expected(measure, rs.codes, rs.codes, row, col)
    assert same_bits(offsets, want[0]) and same_bits(sites, want[1]) and same_bits(bases, want[2])
    assert np.array_equal(np.diff(offsets.astype(np.int64)), POP[rs.xor(row, col)])
    assert same_bits(eng.pair_sites(measure, row, col, count_only=True), want[0])


# ---- h. text ----------------------------------------------------------------------------------------------------------------
def oracle_square_rows(rs, measure, rb, re):
    """the oracle's values of rows [rb, re) of the square, condensed"""
    counts = rs.base_counts().astype(np.uint64)
    full = oracle.all_pairs_rect(measure, rs.codes[rb:re], rs.codes, counts[rb:re], counts, threads=THREADS)
    return np.concatenate([full[r - rb, r + 1:] for r in range(rb, re)])


@pytest.mark.parametrize("rows", [(FIRST_ROW_PAST_2_32 - 2, FIRST_ROW_PAST_2_32 + 3), (65_534, 65_538)])
def test_text_square(eng, rs, rows):
    rb, re = rows
    ids = rs.ids()
    for measure in ("n", "raw", "tn93"):
        want = oracle.tsv_square(measure, oracle_square_rows(rs, measure, rb, re), ids, rb, re, threads=THREADS)
        assert eng.text_square(measure, rb, re, capacity=len(want) + (1 << 16)) == want, measure


def value_texts(measure):
    """what the oracle prints for every value the set holds: texts[d] (n) or texts[3 d + 40 - comparable] (raw)"""
    if measure == "n":
        return [oracle.format_distance(d).encode() for d in range(rbc.BITS + 1)]
    return [oracle.format_distance(float(np.float64(d) / np.float64(c))).encode() for d in range(rbc.BITS + 1) for c in (40, 39, 38)]


def value_codes(rs, measure, r):
    """row r against all records as positions in value_texts"""
    d = POP[rs.words[r] ^ rs.words].astype(np.int64)
    return d if measure == "n" else 3 * d + (40 - rs.comparable(np.full(rs.n, r), np.arange(rs.n)))


@pytest.mark.parametrize("measure", ["n", "raw"])
def test_text_matrix(eng, rs, measure):
    rb, re = 65_530, 65_545
    assert (re - rb) * rs.n < 1 << 31
    ids, texts = rs.ids(), value_texts(measure)
    for style, sep in (("tsv", b"\t"), ("phylip", b" ")):
        want = b"".join(ids[r].encode() + b"".join(sep + texts[c] for c in value_codes(rs, measure, r).tolist()) + b"\n"
                        for r in range(rb, re))
        assert eng.text_matrix(measure, rb, re, style=style, capacity=len(want) + (1 << 16)) == want, style
    # the limits: 23,166 rows of 92,700 cells stay below 2^31 cells, one more row does not
    most = ((1 << 31) - 1) // rs.n
    assert most * rs.n < 1 << 31 <= (most + 1) * rs.n
    with pytest.raises(da.DistanceError):
        eng.text_matrix(measure, 60_000, 60_000 + most + 1, capacity=1 << 10)


@pytest.mark.parametrize("measure", ["n", "raw"])
def test_text_rect(eng, rs, picked_slot, measure):
    """the picked records against the whole set, in ranges of 30 rows: 27.8 million lines"""
    ids, texts = rs.ids(), value_texts(measure)
    col_piece = [i.encode() + b"\t" for i in ids]
    ends = [t + b"\n" for t in texts]
    pieces = [None] * (3 * rs.n)
    pieces[1::3] = col_piece
    for b0 in range(0, len(picked_slot), 30):
        want = []
        for r in picked_slot[b0:b0 + 30]:
            pieces[0::3] = [ids[r].encode() + b"\t"] * rs.n
            pieces[2::3] = map(ends.__getitem__, value_codes(rs, measure, int(r)).tolist())
            want.append(b"".join(pieces))
        want = b"".join(want)
        got = eng.text_rect(measure, 1, 0, b0, min(b0 + 30, len(picked_slot)), capacity=len(want) + (1 << 16))
        assert got == want, (measure, b0)


# ---- i. closest streams -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", ["n", "raw"])
def test_closest_stream_streamed_side(eng, rs, measure):
    """two batches of picked records streamed past the loaded 92,700: every streamed record's 8 nearest loaded records"""
    half = len(rs.picked) // 2
    want_index, want_values = nearest_reference(measure, False)
    with eng.closest_stream(measure, 8, max_records=len(rs.picked), side="streamed", depth=2) as st:
        for lo, hi in ((0, half), (half, len(rs.picked))):
            st.push(rs.codes[rs.picked[lo:hi]])
            index, values, tallies = st.pop()
            assert same_bits(index, want_index[lo:hi, :8]) and same_bits(values, want_values[lo:hi, :8])
            rows = np.repeat(rs.picked[lo:hi], 8)
            assert same_bits(tallies.reshape(len(rows), -1), rs.tallies(measure, rows, index.ravel()).astype(np.uint32))


def test_closest_stream_loaded_side(eng, rs):
    """3 streamed records: every loaded record's 2 nearest of them, ascending (value, streamed ordinal)"""
    streamed = np.array([65_536, FIRST_ROW_PAST_2_32, 17])
    with eng.closest_stream("n", 2, max_records=3, side="loaded", depth=2) as st:
        st.push(rs.codes[streamed])
        assert st.pop() == 3
        index, values = st.result()
    S = np.stack([POP[rs.words[r] ^ rs.words].astype(np.int64) for r in streamed])   # [streamed][loaded]
    order = np.argsort(S * 4 + np.arange(3)[:, None], axis=0)[:2].T                    # [loaded][2]
    assert same_bits(index, order.astype(np.uint32))
    assert same_bits(values, np.take_along_axis(S.T, order, axis=1))


# ---- j. a square slab of more than 65,535 rows: a second launch grid ----------------------------------------------------
def free_device_memory():
    """bytes free on the current device, asked of the HIP runtime the engine has already loaded into this process"""
    with open("/proc/self/maps") as fh:
        paths = {line.split()[-1] for line in fh if "libamdhip64" in line}
    assert paths, "the HIP runtime is not loaded"
    hip = C.CDLL(sorted(paths)[0])
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return int(free.value)


@pytest.fixture(scope="module")
def two_slab_bound(eng, rs):
    """the slab bound of two slabs, the second of 65,539 rows; skips when its 17.2 GB slab does not fit the device"""
    slabs = rbc.cut_row_slabs(rs.n, rbc.TWO_SLAB_MAX_PAIRS)
    assert len(slabs) == 2 and slabs[1][1] - slabs[1][0] > rbc.GRID_ROWS
    need = 8 * max(s[3] for s in slabs) + (8 << 30)   # the larger slab's payloads and a margin
    free = free_device_memory()
    if free < need:
        pytest.skip(f"a slab of {need >> 30} GB with its margin does not fit the device's {free >> 30} GB of free memory")
    return rbc.TWO_SLAB_MAX_PAIRS


@pytest.mark.parametrize("operation", ["links", "clusters", "summary"])
def test_second_row_grid(eng, rs, two_slab_bound, operation):
    """links, clusters and summary over a slab of 65,539 rows, one case each"""
    if operation == "links":
        assert eng.links("n", 2, max_pairs=two_slab_bound, count_only=True) == 860_980
    elif operation == "clusters":
        labels, links = eng.clusters("n", 1, max_pairs=two_slab_bound)
        assert links == 81_846 and same_bits(labels, rs.clusters(1))
    else:
        got = eng.summary("n", 1, max_pairs=two_slab_bound, bins=32, width=1)
        summary_reference.assert_summary(got, square_summary_reference(rs), "two slabs")
