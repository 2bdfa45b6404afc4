"""GPU (-m gpu): the shared preparation (dst_upload_shared) on designed lists, rank cuts and block fits.

shared_structure_cases.py lays out the sets and test_shared_structure_host.py holds them to their design: list lengths of
0 ... 193 entries around the 64-lane rounds of range_marks_kernel, lists that skip ranges or lie in the last range or in
range 0 only, 65 ranges, feature records either side of every rank cut of world 2 ... 5, shares of one record and of
none, a share of exactly the first block's 40,960 entries and of 40,961, a block sized from a smaller set, the `diverse`
and `hot_columns` fallbacks, and the census of list_structure_cases.py (without its hot columns) built from exchanged
lists and recomputed marks.  The ranks are threads with one context each on GPU 0 (shared_ranks.py), five at most.

Tallies and the n / jc69 / k80 / tn93 distances are compared bit for bit with the dense kernels of a pristine single
context on the same codes (closed before the ranks start); whole rows of the feature records with the oracle: tallies
exact, distances at 1e-12.  Where the whole triangle of a large set is compared inside the rank threads, the same rows of
the dense result are held to the oracle instead, which ties the ranks' rows to it through the bitwise comparison.  The
closing tests run what a partial set serves besides run_square (a rectangle with it as columns, streams, the slab
analyses, matrix text) and hold every call it must refuse to DST_ERR_STATE with the context usable afterwards."""
import numpy as np
import pytest

import distance_amd as da
import list_structure_cases as ls
import oracle
import shared_structure_cases as sc
from shared_ranks import ThreadRanks

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FAMILIES = ("n_high", "raw", "k80", "tn93")
DISTANCES = ("n", "jc69", "k80", "tn93")
ERR_STATE = 4
TOL = 1e-12


def rows_of_triangle(tri, n, rows):
    """(len(rows), n, ...) whole rows out of a canonical triangle (the diagonal takes pair 0: masked by the callers)"""
    r = np.asarray(rows, np.int64)[:, None]
    j = np.arange(n, dtype=np.int64)[None, :]
    a, b = np.minimum(r, j), np.maximum(r, j)
    idx = a * (2 * n - a - 1) // 2 + b - a - 1
    idx[r == j] = 0
    return tri[idx]


def off_diagonal(rows, n):
    return np.asarray(rows)[:, None] != np.arange(n)[None, :]


def assert_close(got, want):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "NaN pattern differs"
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), "inf pattern differs"
    ok = ~(nan | inf)
    err = np.abs(got[ok] - want[ok])
    assert np.all(err <= TOL), f"abs err {err.max()}"
    big = np.abs(want[ok]) >= 1e-3
    assert np.all(err[big] <= TOL * np.abs(want[ok][big])), f"rel err {(err[big] / np.abs(want[ok][big])).max()}"


def dense_of(codes, families=FAMILIES, distances=DISTANCES, partner=None):
    """the dense kernels of a pristine engine, closed again before any rank starts"""
    out = {"t": {}, "d": {}, "r10": {}, "r10d": {}}
    with da.Engine(0) as ref:
        ref.set_path("dense")
        ref.upload(0, codes)
        for m in families:
            out["t"][m] = ref.run_square(m, tallies=True)
        for m in distances:
            out["d"][m] = ref.run_square(m)
        if partner is not None:
            ref.upload(1, partner)
            for m in FAMILIES:
                out["r10"][m] = ref.run_rect(m, 1, 0, tallies=True)
            for m in ("n_high", "tn93"):
                out["r10d"][m] = ref.run_rect(m, 1, 0)
        assert ref.last_path() == "dense"
    return out


def on_device(codes):
    d = torch.from_numpy(codes).cuda()
    return d, (d.data_ptr(), codes.shape[0], codes.shape[1], d.stride(0))


def slice_of(n, r0, r1):
    return slice(da.square_row_start(n, r0), da.square_row_start(n, r1))


def compare_rows(eng, n, r0, r1, dense, families=FAMILIES, distances=DISTANCES, what=""):
    """rows [r0, r1) of every family and distance against the dense triangle, bit for bit; returns the tallies"""
    sl, got = slice_of(n, r0, r1), {}
    for m in families:
        got[m] = eng.run_square(m, r0, r1, tallies=True)
        assert np.array_equal(got[m], dense["t"][m][sl]), (what, m, r0, r1)
    for m in distances:
        got["d_" + m] = eng.run_square(m, r0, r1)
        assert np.array_equal(got["d_" + m], dense["d"][m][sl], equal_nan=True), (what, m, r0, r1)
    return got


def rows_against_oracle(codes, rows, tri_t, tri_d):
    """whole rows of a canonical triangle against the oracle: tallies exact, distances at 1e-12"""
    n = len(codes)
    rows = sorted(set(int(r) for r in rows))
    sub, off = np.ascontiguousarray(codes[rows]), off_diagonal(rows, n)
    for m, tri in tri_t.items():
        want = oracle.tallies_rect(m, sub, codes, threads=8)
        assert np.array_equal(rows_of_triangle(tri, n, rows)[off], want[off]), m
    for m, tri in tri_d.items():
        if m == "n":
            continue
        assert_close(rows_of_triangle(tri, n, rows)[off], oracle.all_pairs_rect(m, sub, codes, threads=8)[off])


def refused(call):
    with pytest.raises(da.DistanceError) as e:
        call()
    assert e.value.status == ERR_STATE, (e.value.status, e.value.message)


# ---------------------------------------------------------------------------------------------------------------------
# cut_set: every rank cut of world 2 ... 5
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cut():
    codes, names = sc.cut_set()
    partner = ls.partner_alignment(names["root"])
    c = ls.census(codes)
    return {"codes": codes, "names": names, "partner": partner, "length": c["length"], "dense": dense_of(codes, partner=partner),
            "counts": oracle.count_bases_matrix(codes).astype(np.uint32)}


def cut_ranges(n, world):
    """row ranges that start and end exactly at a rank cut, and one record either side of it"""
    out = []
    for b, _ in sc.shares(n, world):
        if 0 < b < n:
            out += [(b - 1, b), (b, b + 1), (b - 1, b + 1), (max(b - 256, 0), b), (b, min(b + 9, n))]
    return out


@pytest.mark.parametrize("prep", ("default", "fused"))
@pytest.mark.parametrize("world", (2, 3, 4, 5))
def test_cut_set_on_every_rank_cut(cut, world, prep):
    codes, dense, n = cut["codes"], cut["dense"], sc.CUT_N
    dcodes, where = on_device(codes)
    bounds = da.partition_square(n, world)
    biggest = max(sc.share_totals(cut["length"], n, world))

    def body(rank, eng, comm):
        if prep == "fused":
            eng.set_prep_threshold(0.0)
        eng.upload_shared(comm, 0, *where, with_counts=True)
        assert eng.shared_stats() == {"shared_uploads": 1, "fallbacks": 0, "block_entries": biggest}
        got = compare_rows(eng, n, bounds[rank], bounds[rank + 1], dense, what=(world, rank))
        assert eng.last_path() == "consensus"
        assert np.array_equal(eng.base_counts(0), cut["counts"]), (world, rank)
        for r0, r1 in cut_ranges(n, world):
            compare_rows(eng, n, r0, r1, dense, ("raw", "tn93"), ("n", "tn93"), what=(world, rank))
        assert eng.last_path() == "consensus"
        return got

    res = ThreadRanks(world).run(body)
    # the ranks' ranges, end to end, are the triangle: the feature rows of it against the oracle
    tri_t = {m: np.concatenate([r[m] for r in res]) for m in FAMILIES}
    tri_d = {m: np.concatenate([r["d_" + m] for r in res]) for m in DISTANCES}
    assert all(len(tri_t[m]) == n * (n - 1) // 2 for m in FAMILIES)
    if prep == "default":
        rows_against_oracle(codes, cut["names"]["features"], tri_t, tri_d)


# ---------------------------------------------------------------------------------------------------------------------
# the block fit: 40,960 entries against 40,961, and a block sized from a smaller set
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fit():
    fits, over, _ = sc.fit_sets()
    return {"fits": fits, "over": over, "dense_fits": dense_of(fits), "dense_over": dense_of(over)}


def test_a_share_of_exactly_the_first_capacity_fits(fit):
    n, bounds = sc.FIT_N, da.partition_square(sc.FIT_N, 2)
    d, where = on_device(fit["fits"])

    def body(rank, eng, comm):
        eng.upload_shared(comm, 0, *where, with_counts=True)
        assert eng.shared_stats() == {"shared_uploads": 1, "fallbacks": 0, "block_entries": 40960}
        compare_rows(eng, n, bounds[rank], bounds[rank + 1], fit["dense_fits"])
        assert eng.last_path() == "consensus"
        compare_rows(eng, n, 254, 258, fit["dense_fits"], ("tn93",), ("tn93",))      # either side of the cut at 256

    ThreadRanks(2).run(body)


def test_one_entry_more_falls_back_on_both_ranks_then_fits(fit):
    n, bounds = sc.FIT_N, da.partition_square(sc.FIT_N, 2)
    d, where = on_device(fit["over"])

    def body(rank, eng, comm):
        eng.upload_shared(comm, 0, *where, with_counts=True)
        assert eng.shared_stats() == {"shared_uploads": 0, "fallbacks": 1, "block_entries": 40961}
        compare_rows(eng, n, bounds[rank], bounds[rank + 1], fit["dense_over"])
        compare_rows(eng, n, 254, 258, fit["dense_over"], ("tn93",), ("tn93",))
        # the next block is sized from what the headers said
        eng.upload_shared(comm, 0, *where, with_counts=True)
        assert eng.shared_stats() == {"shared_uploads": 1, "fallbacks": 1, "block_entries": 40961}
        compare_rows(eng, n, bounds[rank], bounds[rank + 1], fit["dense_over"])
        assert eng.last_path() == "consensus"
        compare_rows(eng, n, 254, 258, fit["dense_over"], ("tn93",), ("tn93",))

    ThreadRanks(2).run(body)


def test_a_block_sized_from_a_smaller_set_falls_back_then_fits(cut, fit):
    n, bounds = sc.FIT_N, da.partition_square(sc.FIT_N, 2)
    small = np.ascontiguousarray(cut["codes"][:512])
    dense_small = dense_of(small, ("raw", "tn93"), ("tn93",))
    biggest = max(sc.share_totals(cut["length"][:512], 512, 2))
    ds, where_small = on_device(small)
    d, where = on_device(fit["fits"])

    def body(rank, eng, comm):
        eng.upload_shared(comm, 0, *where_small, with_counts=True)
        assert eng.shared_stats() == {"shared_uploads": 1, "fallbacks": 0, "block_entries": biggest}
        compare_rows(eng, n, bounds[rank], bounds[rank + 1], dense_small, ("raw", "tn93"), ("tn93",))
        eng.upload_shared(comm, 0, *where, with_counts=True)
        assert eng.shared_stats() == {"shared_uploads": 1, "fallbacks": 1, "block_entries": 40960}
        compare_rows(eng, n, bounds[rank], bounds[rank + 1], fit["dense_fits"])
        eng.upload_shared(comm, 0, *where, with_counts=True)
        assert eng.shared_stats() == {"shared_uploads": 2, "fallbacks": 1, "block_entries": 40960}
        compare_rows(eng, n, bounds[rank], bounds[rank + 1], fit["dense_fits"])
        assert eng.last_path() == "consensus"

    ThreadRanks(2).run(body)


# ---------------------------------------------------------------------------------------------------------------------
# the fallbacks: a set past the 8 % gate, hot columns that carry weight
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,world", (("diverse", 3), ("hot_columns", 2)))
def test_fallbacks_are_taken_together_and_a_benign_set_rides_again(cut, which, world):
    codes = sc.diverse_set() if which == "diverse" else ls.census_alignment()[0]
    n = len(codes)
    dense = dense_of(codes, ("raw",), ("tn93",))
    d, where = on_device(codes)
    dcut, where_cut = on_device(cut["codes"])
    bounds, cut_bounds = da.partition_square(n, world), da.partition_square(sc.CUT_N, world)
    biggest = max(sc.share_totals(cut["length"], sc.CUT_N, world))

    def body(rank, eng, comm):
        eng.upload_shared(comm, 0, *where, with_counts=True)
        st = eng.shared_stats()
        assert st["shared_uploads"] == 0 and st["fallbacks"] == 1, st
        r0, r1 = bounds[rank], bounds[rank + 1]
        compare_rows(eng, n, r0, r1, dense, ("raw",), ("tn93",), what=which)
        eng.set_path("dense")                       # the replicated upload holds every record's planes
        compare_rows(eng, n, r0, min(r0 + 40, r1), dense, ("raw",), ("tn93",), what=which)
        assert eng.last_path() == "dense"
        eng.set_path("auto")
        eng.upload_shared(comm, 0, *where_cut, with_counts=True)
        st = eng.shared_stats()
        assert st["shared_uploads"] == 1 and st["fallbacks"] == 1, st
        if which == "hot_columns":                  # (the diverse set's blocks were larger: the headers said so)
            assert st["block_entries"] == biggest
        compare_rows(eng, sc.CUT_N, cut_bounds[rank], cut_bounds[rank + 1], cut["dense"], what=which)
        assert eng.last_path() == "consensus"
        assert np.array_equal(eng.base_counts(0), cut["counts"])

    ThreadRanks(world).run(body)


# ---------------------------------------------------------------------------------------------------------------------
# the census without its hot columns: buckets, overflows, slots, pieces, batches and runs from exchanged lists
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cooled():
    codes, names = sc.cooled_census()
    return {"codes": codes, "names": names, "dense": dense_of(codes), "counts": oracle.count_bases_matrix(codes).astype(np.uint32)}


def test_the_dense_rows_of_the_cooled_census_are_the_oracles(cooled):
    names = cooled["names"]
    rows = set(names["probes"].values()) | {r for pair in names["batches_cold"] for r in pair} | set(names["runs"].values())
    rows |= {0, 1535, 1536, 2303, 2304, 3071, 3072, 4395}
    rows_against_oracle(cooled["codes"], rows, cooled["dense"]["t"], cooled["dense"]["d"])


@pytest.mark.parametrize("world", (2, 3))
def test_cooled_census_from_exchanged_lists(cooled, world):
    codes, dense, n = cooled["codes"], cooled["dense"], ls.N_RECORDS
    d, where = on_device(codes)
    bounds = da.partition_square(n, world)
    biggest = max(sc.share_totals(ls.census(codes)["length"], n, world))

    def body(rank, eng, comm):
        eng.upload_shared(comm, 0, *where, with_counts=True)
        assert eng.shared_stats() == {"shared_uploads": 1, "fallbacks": 0, "block_entries": biggest}
        r0, r1 = bounds[rank], bounds[rank + 1]
        sl = slice_of(n, r0, r1)
        for m in FAMILIES:                           # (compared and dropped: a family's triangle is up to 150 MB)
            assert np.array_equal(eng.run_square(m, r0, r1, tallies=True), dense["t"][m][sl]), (world, rank, m)
        for m in DISTANCES:
            assert np.array_equal(eng.run_square(m, r0, r1), dense["d"][m][sl], equal_nan=True), (world, rank, m)
        assert eng.last_path() == "consensus"
        assert np.array_equal(eng.base_counts(0), cooled["counts"]), (world, rank)

    ThreadRanks(world).run(body)


# ---------------------------------------------------------------------------------------------------------------------
# 65 ranges, and the small sets
# ---------------------------------------------------------------------------------------------------------------------
def test_wide_cut_set_marks_65_ranges():
    codes, names = sc.wide_cut_set()
    n = len(codes)
    dense = dense_of(codes, FAMILIES, ("n", "tn93"))
    d, where = on_device(codes)
    bounds = da.partition_square(n, 2)
    biggest = max(sc.share_totals(ls.census(codes)["length"], n, 2))

    def body(rank, eng, comm):
        eng.upload_shared(comm, 0, *where, with_counts=True)
        assert eng.shared_stats() == {"shared_uploads": 1, "fallbacks": 0, "block_entries": biggest}
        got = compare_rows(eng, n, bounds[rank], bounds[rank + 1], dense, FAMILIES, ("n", "tn93"))
        assert eng.last_path() == "consensus" and eng.last_launch()["wide"]
        return got

    res = ThreadRanks(2).run(body)
    tri_t = {m: np.concatenate([r[m] for r in res]) for m in FAMILIES}
    tri_d = {"tn93": np.concatenate([r["d_tn93"] for r in res])}
    rows_against_oracle(codes, names["added"].values(), tri_t, tri_d)


@pytest.mark.parametrize("n,world", ((2, 2), (257, 2), (300, 3)))
def test_small_sets_with_shares_of_one_record_and_of_none(n, world):
    codes = sc.small_set(n)
    dense = dense_of(codes)
    d, where = on_device(codes)
    bounds = da.partition_square(n, world)
    biggest = max(sc.share_totals(ls.census(codes)["length"], n, world))
    counts = oracle.count_bases_matrix(codes).astype(np.uint32)

    def body(rank, eng, comm):
        eng.upload_shared(comm, 0, *where, with_counts=True)
        assert eng.shared_stats() == {"shared_uploads": 1, "fallbacks": 0, "block_entries": biggest}
        got = compare_rows(eng, n, bounds[rank], bounds[rank + 1], dense, what=(n, world, rank))
        if bounds[rank + 1] > bounds[rank]:
            assert eng.last_path() == "consensus"
        assert np.array_equal(eng.base_counts(0), counts)
        return got

    res = ThreadRanks(world).run(body)
    tri_t = {m: np.concatenate([r[m] for r in res]) for m in FAMILIES}
    tri_d = {m: np.concatenate([r["d_" + m] for r in res]) for m in DISTANCES}
    rows_against_oracle(codes, range(n), tri_t, tri_d)               # the whole triangle


# ---------------------------------------------------------------------------------------------------------------------
# what a partial set serves besides run_square, and what it refuses
# ---------------------------------------------------------------------------------------------------------------------
def stream_all(eng, measure, partner, nibbles):
    got = []
    with eng.stream(measure, max_records=48, depth=3, nibbles=nibbles) as st:
        for b0 in range(0, len(partner), 48):                        # 48, 48 and 34 records
            if st.in_flight() == 2:
                got.append(st.pop())
            st.push(partner[b0:b0 + 48])
        while st.in_flight():
            got.append(st.pop())
    return np.concatenate(got)


def analyses(eng, rows):
    """the slab analyses and the matrix text of slot 0, as comparable pieces"""
    out = {}
    out["links_n"] = eng.links("n", 5, tallies=True)
    out["links_tn93"] = eng.links("tn93", 0.0012)
    out["clusters"] = eng.clusters("n", 4)
    s = eng.summary("tn93", threshold=0.0012, bins=16, width=0.0005)
    out["summary"] = tuple(s[k] for k in sorted(s))
    out["nearest"] = eng.nearest("tn93", 8, tallies=True)
    out["nearest_n"] = eng.nearest("n", 8)
    out["mst"] = eng.mst("tn93")
    out["text"] = (eng.text_matrix("tn93", rows[0], rows[1]), eng.text_matrix("n", rows[0], rows[1], style="phylip"))
    return out


def same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
    if isinstance(a, float):
        return a == b or (a != a and b != b)
    return a == b


def test_what_a_partial_set_serves(cut):
    codes, partner, dense, n = cut["codes"], cut["partner"], cut["dense"], sc.CUT_N
    ids = ["r%d" % k for k in range(n)]
    row_ranges = [(760, 776), (0, 12)]
    with da.Engine(0) as plain:                     # a single plain context's answers
        plain.upload(0, codes)
        plain.upload(1, partner)
        plain.set_ids(0, ids)
        want = [analyses(plain, rows) for rows in row_ranges]
        want_stream = {(m, nib): stream_all(plain, m, partner, nib) for m in ("n_high", "tn93") for nib in (False, True)}
    oracle_t = {m: oracle.tallies_rect(m, partner, codes, threads=8) for m in FAMILIES}
    oracle_tn93 = oracle.all_pairs_rect("tn93", partner, codes, threads=8)
    for nib in (False, True):
        assert np.array_equal(want_stream[("n_high", nib)], oracle_t["n_high"][..., 0].astype(np.int64))
        assert_close(want_stream[("tn93", nib)], oracle_tn93)
    d, where = on_device(codes)

    def body(rank, eng, comm):
        eng.upload_shared(comm, 0, *where, with_counts=True)
        eng.upload(1, partner)
        eng.set_ids(0, ids)
        assert eng.shared_stats()["shared_uploads"] == 1
        # a rectangle with the shared set as columns: the partner's lists against the shared set's reference
        for m in FAMILIES:
            got = eng.run_rect(m, 1, 0, tallies=True)
            assert eng.last_path() == "consensus"
            assert np.array_equal(got, dense["r10"][m]) and np.array_equal(got, oracle_t[m].astype(np.uint32)), m
        for m in ("n_high", "tn93"):
            assert np.array_equal(eng.run_rect(m, 1, 0), dense["r10d"][m], equal_nan=True), m
        # a stream against it, bytes and nibbles
        for key, w in want_stream.items():
            assert same(stream_all(eng, key[0], partner, key[1]), w), key
            assert eng.last_path() == "consensus"
        # the slab analyses and the matrix text
        got = analyses(eng, row_ranges[rank])
        for key, w in want[rank].items():
            assert same(got[key], w), (rank, key)
        assert eng.last_path() == "consensus"
        return len(got["links_n"][0]), len(got["links_tn93"][0]), got["clusters"][1]

    for n_links, n_links_f, cl_links in ThreadRanks(2).run(body):
        assert 0 < n_links < n * (n - 1) // 2 and 0 < n_links_f < n * (n - 1) // 2 and cl_links > 0


def test_what_a_partial_set_refuses(cut):
    codes, partner, dense, n = cut["codes"], cut["partner"], cut["dense"], sc.CUT_N
    d, where = on_device(codes)
    second = np.ascontiguousarray(codes[:130])      # (the partner's own hot columns would send its shared upload back)
    dp, where_second = on_device(second)
    consensus = oracle.consensus(codes)

    def body(rank, eng, comm):
        def usable():
            r0 = 255 + 512 * rank
            compare_rows(eng, n, r0, r0 + 2, dense, ("raw",), ("jc69",))
            assert eng.last_path() == "consensus"

        eng.upload_shared(comm, 0, *where, with_counts=True)
        eng.upload(1, partner)
        usable()
        for call in (lambda: eng.run_rect("raw", 0, 1, tallies=True),           # shared rows against another set's reference
                     lambda: eng.pair_sites("raw", [0, 3], [1, 2]),
                     lambda: eng.pair_sites("raw", [0], [1], square=False, row_slot=1, col_slot=0),
                     lambda: eng.consensus(),
                     lambda: eng.consensus(both_slots=True),
                     lambda: eng.differences(0, codes[0])):
            refused(call)
            usable()
        for path in ("dense", "hybrid"):
            eng.set_path(path)
            refused(lambda: eng.run_square("raw", 0, 4, tallies=True))
            refused(lambda: eng.run_rect("raw", 1, 0, tallies=True))
            eng.set_path("auto")
            usable()
        # both slots shared: neither order of the rectangle has a row set whose lists can be rebuilt
        eng.upload_shared(comm, 1, *where_second, with_counts=True)
        assert eng.shared_stats(1) == {"shared_uploads": 1, "fallbacks": 0, "block_entries": int(cut["length"][:130].sum())}
        refused(lambda: eng.run_rect("raw", 0, 1, tallies=True))
        refused(lambda: eng.run_rect("raw", 1, 0, tallies=True))
        usable()
        # no base counts came with the exchange: tn93 distances need them, its tallies do not
        eng.upload_shared(comm, 0, *where)
        assert eng.shared_stats()["shared_uploads"] == 2
        refused(lambda: eng.run_square("tn93", 0, 4))
        compare_rows(eng, n, 509, 514, dense, ("tn93", "raw"), ("k80",))
        # a plain upload to the same slot clears it
        eng.upload(0, codes)
        eng.set_path("dense")
        compare_rows(eng, n, 509, 514, dense, FAMILIES, DISTANCES)
        assert eng.last_path() == "dense"
        eng.set_path("auto")
        offsets, sites, bases = eng.pair_sites("raw", [0, 3], [1, 2])
        assert int(offsets[-1]) == len(sites) == len(bases) == int(dense["t"]["raw"][0][0] + dense["t"]["raw"][slice_of(n, 2, 3)][0][0])
        assert np.array_equal(eng.consensus(), consensus)
        assert len(eng.differences(0, codes[0])) == n

    ThreadRanks(2).run(body)
