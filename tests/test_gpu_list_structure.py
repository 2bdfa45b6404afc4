"""GPU (-m gpu): every slot, piece, bucket, batch and run-record boundary of the consensus path's lists, on designed sets.

list_structure_cases.py lays out one alignment (4,396 x 4,200: two full panels and one of 300 records) with a named size on
either side of every boundary between an upload and a result — pack slots of 7 / 8 differences, list pieces of 8 / 9 and
72 / 73 entries, buckets of 15 / 16 entries and overflows of 63 ... 129, batches of 64 EW - 1 ... 64 EW + 1 entries, records
of 3 / 4 run chunks — and test_list_structure_host.py holds the layout to a census taken from the code matrix alone.  Here
the set goes through consensus / hybrid / auto under the fused and the plain preparation: the whole triangle of all four
tally families and of the n / jc69 / k80 / tn93 distances bit for bit against the dense kernels of a pristine engine (which
know nothing of lists), whole rows of the feature records against the oracle, row ranges that move and cut the batches,
rectangles in both slot orders against a partner set (lists against another set's reference), a streamed batch, the
difference sites of feature pairs, the wide form of the same records, and the run-table sets (n_run = 1 ... 234 of 700
records, 256 and 257 chunks).  Every launch's dst_last_launch is recorded; the closing test holds what was seen.

At this size the default preparation threshold (2e10 site comparisons) already sends the upload through the fused
preparation, so the second preparation here is the plain one (threshold 1e30: lists built from the planes at the first
run), not the default."""
import numpy as np
import pytest

import distance_amd as da
import list_structure_cases as ls
import oracle
import pair_sites_reference as psr

pytestmark = pytest.mark.gpu
FAMILIES = ("n_high", "raw", "k80", "tn93")
DISTANCES = ("n", "jc69", "k80", "tn93")
PATHS = ("consensus", "hybrid", "auto")
PREPS = {"fused": 0.0, "plain": 1e30}
TOL = 1e-12
SEEN = {"ew": set(), "rows_per_tile": set(), "hot_columns": set(), "run_records": set(), "paths": set(), "launches": 0,
        "by_ew": {}}


@pytest.fixture(scope="module")
def eng():
    e = da.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def design():
    codes, names = ls.census_alignment()
    ref, dev, hot = ls.sampled_reference(codes)
    c = ls.census(codes, ref)
    return {"codes": codes, "names": names, "hot": hot, "length": c["length"],
            "cold": (c["diff"] & ~hot[None, :]).sum(axis=1), "partner": ls.partner_alignment(names["root"])}


@pytest.fixture(scope="module")
def dense(design):
    """the dense kernels of a pristine engine: the whole triangle and both rectangles"""
    out = {"t": {}, "d": {}, "r01": {}, "r10": {}}
    with da.Engine(0) as ref:
        ref.set_path("dense")
        ref.upload(0, design["codes"])
        ref.upload(1, design["partner"])
        for m in FAMILIES:
            out["t"][m] = ref.run_square(m, tallies=True)
            out["r01"][m] = ref.run_rect(m, 0, 1, tallies=True)
            out["r10"][m] = ref.run_rect(m, 1, 0, tallies=True)
        for m in DISTANCES:
            out["d"][m] = ref.run_square(m)
        assert ref.last_path() == "dense"
    return out


@pytest.fixture(scope="module")
def oracle_rows(design):
    """whole rows of the feature records by the oracle: every probe and batch row, the panels' first and last records, the
    run records, and one record of every slot and piece size"""
    codes, names = design["codes"], design["names"]
    rows = set(names["probes"].values()) | {r for pair in list(names["batches"]) + list(names["batches_cold"]) for r in pair}
    rows |= set(names["runs"].values()) | set(range(0, 18)) | {2047, 2048, 4095, 4096, 4395} | set(range(4097, 4113))
    rows = sorted(rows)
    sub = np.ascontiguousarray(codes[rows])
    return {"rows": rows, "t": {m: oracle.tallies_rect(m, sub, codes, threads=8) for m in FAMILIES},
            "d": {m: oracle.all_pairs_rect(m, sub, codes, threads=8) for m in ("jc69", "k80", "tn93")}}


@pytest.fixture(scope="module")
def oracle_partner(design):
    return {m: oracle.tallies_rect(m, design["partner"], design["codes"], threads=8) for m in FAMILIES}


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


def note(eng, design=None, whole=False):
    """record the launch; a whole-triangle launch of the census set must have had a batch of 64 EW - 1, 64 EW and 64 EW + 1
    entries among its rows (the hybrid path's lists are without the hot columns)"""
    li = eng.last_launch()
    SEEN["launches"] += 1
    SEEN["paths"].add(li["path"])
    if li["path"] == "dense":
        return li
    SEEN["ew"].add(li["event_waves"])
    SEEN["by_ew"].setdefault(li["event_waves"], set()).add("%s %s %s" % (li["path"], li["measure"], "tallies" if li["out_kind"] else "values"))
    SEEN["rows_per_tile"].add(li["rows_per_tile"])
    if whole:
        length = design["cold"] if li["path"] == "hybrid" else design["length"]
        SEEN["hot_columns"].add(int(design["hot"].sum()) if li["path"] == "hybrid" else 0)
        sums = set(ls.batch_sums(length, 0, ls.N_RECORDS, li["rows_per_tile"], ls.PANEL - 1))
        ew = li["event_waves"]
        assert {64 * ew - 1, 64 * ew, 64 * ew + 1} <= sums, li
    return li


def prepare(eng, prep, codes, expect_runs):
    eng.set_prep_threshold(PREPS[prep])
    eng.set_path("auto")
    eng.upload(0, codes)
    if prep == "fused":
        assert not eng.planes_stored(0)             # the slots really built the lists
        assert eng.run_records()[0] == expect_runs
    else:
        assert eng.planes_stored(0) and eng.run_records()[0] == 0
    SEEN["run_records"].add(eng.run_records()[0])


def restore(eng):
    eng.set_prep_threshold(2e10)
    eng.set_path("auto")


def test_the_default_threshold_is_the_fused_preparation_here(eng, design):
    eng.set_path("auto")
    eng.upload(0, design["codes"])
    assert not eng.planes_stored(0) and eng.run_records()[0] == 3


@pytest.mark.parametrize("prep", PREPS)
@pytest.mark.parametrize("path", PATHS)
def test_whole_triangle_against_dense_and_oracle(eng, design, dense, oracle_rows, path, prep):
    codes, n = design["codes"], ls.N_RECORDS
    rows, off = oracle_rows["rows"], off_diagonal(oracle_rows["rows"], ls.N_RECORDS)
    try:
        prepare(eng, prep, codes, 3)
        eng.set_path(path)
        for m in FAMILIES:
            got = eng.run_square(m, tallies=True)
            li = note(eng, design, whole=True)
            assert np.array_equal(got, dense["t"][m]), (path, prep, m, li)
            assert np.array_equal(rows_of_triangle(got, n, rows)[off], oracle_rows["t"][m][off]), (path, prep, m)
        if path != "auto":
            assert eng.last_path() == path
        for m in DISTANCES:
            got = eng.run_square(m)
            li = note(eng, design, whole=True)
            assert np.array_equal(got, dense["d"][m], equal_nan=True), (path, prep, m, li)
            if m in oracle_rows["d"]:
                assert_close(rows_of_triangle(got, n, rows)[off], oracle_rows["d"][m][off])
        if path != "auto":
            assert eng.last_path() == path
        # row ranges: from row 33 the batches pair the rows the other way, (32, 33) is a tile of one row, and a range that
        # ends inside a tile leaves a batch of a single row behind
        for rb, re in ((33, 60), (32, 33), (0, 45)):
            a, b = da.square_row_start(n, rb), da.square_row_start(n, re)
            for m in ("raw", "tn93"):
                assert np.array_equal(eng.run_square(m, rb, re, tallies=True), dense["t"][m][a:b]), (path, prep, m, rb, re)
                note(eng)
            assert np.array_equal(eng.run_square("jc69", rb, re), dense["d"]["jc69"][a:b], equal_nan=True), (path, prep, rb, re)
            note(eng)
    finally:
        restore(eng)


@pytest.mark.parametrize("prep", PREPS)
@pytest.mark.parametrize("path", ("consensus", "hybrid"))
def test_rectangles_in_both_slot_orders_and_a_streamed_batch(eng, design, dense, oracle_partner, path, prep):
    codes, partner = design["codes"], design["partner"]
    try:
        prepare(eng, prep, codes, 3)
        eng.upload(1, partner)
        eng.set_path(path)
        for m in FAMILIES:
            want = oracle_partner[m].astype(np.uint32)
            got = eng.run_rect(m, 0, 1, tallies=True)           # the census's rows against the partner's reference
            note(eng)
            assert np.array_equal(got, dense["r01"][m]), (path, prep, m)
            assert np.array_equal(got, want.transpose(1, 0, 2)), (path, prep, m)
            got = eng.run_rect(m, 1, 0, tallies=True)           # the partner's rows probe the buckets of every panel
            note(eng)
            assert np.array_equal(got, dense["r10"][m]), (path, prep, m)
            assert np.array_equal(got, want), (path, prep, m)
            assert eng.last_path() == path
        eng.set_path("consensus")
        for m in FAMILIES:
            got = eng.run_stream_batch(m, partner[:8], tallies=True)
            note(eng)
            assert eng.last_path() == "consensus"
            assert np.array_equal(got, oracle_partner[m][:8].astype(np.uint32)), (prep, m)
            assert np.array_equal(got, dense["r10"][m][:8]), (prep, m)
    finally:
        restore(eng)


def test_the_difference_sites_of_feature_pairs(eng, design):
    """an independent reading of the same planes after a deferring upload"""
    codes, names = design["codes"], design["names"]
    rng = np.random.default_rng(11)
    feat = np.array(names["features"])
    row, col = rng.choice(feat, 300), rng.choice(feat, 300)
    try:
        prepare(eng, "fused", codes, 3)
        eng.set_path("consensus")
        for m in ("raw", "k80", "tn93"):
            offsets, sites, bases = eng.pair_sites(m, row, col)
            want = psr.expected(m, codes, codes, row, col)
            assert np.array_equal(offsets, want[0]) and np.array_equal(sites, want[1]) and np.array_equal(bases, want[2]), m
    finally:
        restore(eng)


def test_the_wide_form(eng, design):
    """the same feature records with one tally per word (65,664 sites, 513 chunks)"""
    wide, keep = ls.wide_form(design["codes"], design["names"])
    with da.Engine(0) as ref:
        ref.set_path("dense")
        ref.upload(0, wide)
        want = {m: ref.run_square(m, tallies=True) for m in FAMILIES}
    try:
        eng.set_prep_threshold(0.0)
        eng.set_path("auto")
        eng.upload(0, wide)
        assert not eng.planes_stored(0) and eng.run_records()[0] >= 1
        eng.set_path("consensus")
        for m in FAMILIES:
            assert np.array_equal(eng.run_square(m, tallies=True), want[m]), m
            li = note(eng)
            assert li["wide"] and eng.last_path() == "consensus"
    finally:
        restore(eng)


def run_table_case(eng, codes, expect_runs, families, distances, oracle_rows_of):
    n = len(codes)
    with da.Engine(0) as ref:
        ref.set_path("dense")
        ref.upload(0, codes)
        want_t = {m: ref.run_square(m, tallies=True) for m in families}
        want_d = {m: ref.run_square(m) for m in distances}
    try:
        eng.set_prep_threshold(0.0)
        eng.set_path("auto")
        eng.upload(0, codes)
        assert not eng.planes_stored(0)
        eng.set_path("consensus")
        got_t = {}
        for m in families:
            got_t[m] = eng.run_square(m, tallies=True)
            li = note(eng)
            assert np.array_equal(got_t[m], want_t[m]), m
            assert li["run_records"] == (expect_runs > 0), li
        for m in distances:
            assert np.array_equal(eng.run_square(m), want_d[m], equal_nan=True), m
            note(eng)
        assert eng.last_path() == "consensus"
        assert eng.run_records()[0] == expect_runs
        SEEN["run_records"].add(expect_runs)
    finally:
        restore(eng)
    rows = oracle_rows_of
    sub = np.ascontiguousarray(codes[rows])
    off = off_diagonal(rows, n)
    for m in families:
        want = oracle.tallies_rect(m, sub, codes, threads=8)
        assert np.array_equal(rows_of_triangle(got_t[m], n, rows)[off], want[off]), m


@pytest.mark.parametrize("n_run", ls.RUN_TABLE_N_RUN)
def test_run_table_sets(eng, n_run):
    """1, 32 / 33 and 128 / 129 run records (one MFMA tile and one block, and one more), 233 = n / 3 (the most that are
    stripped) and 234 (none is)"""
    codes = ls.run_table_alignment(n_run)
    rows = sorted({0, 1, n_run - 1, min(n_run, 698), 31, 32, 350, 699})[:8]
    run_table_case(eng, codes, n_run if n_run <= 233 else 0, FAMILIES, DISTANCES, rows)


@pytest.mark.parametrize("L", (32768, 32896))
def test_long_run_table_sets(eng, L):
    """256 and 257 chunks: eight mask words, and a ninth"""
    codes = ls.run_table_alignment(40, n=300, L=L, n_class_every=16, seed=L)
    run_table_case(eng, codes, 40, ("tn93", "raw"), (), [0, 1, 38, 39, 40, 150, 298, 299])


def test_what_the_launches_showed():
    """closing: the event-wave counts, tile heights, hot-column counts and run-record counts the module's launches had"""
    print("list structure launches:", {k: sorted(v, key=str) if isinstance(v, set) else v for k, v in SEEN.items() if k != "by_ew"})
    for ew, what in sorted(SEEN["by_ew"].items()):
        print("  EW = %d:" % ew, ", ".join(sorted(what)))
    missing = {2, 4, 8} - SEEN["ew"]
    assert not missing, f"no launch of this module ran with EW = {sorted(missing)} (seen: {sorted(SEEN['ew'])})"
    assert {"consensus", "hybrid"} <= SEEN["paths"]
    assert {0, 6} <= SEEN["hot_columns"]
    assert {0, 1, 3, 32, 33, 40, 128, 129, 233} <= SEEN["run_records"]
