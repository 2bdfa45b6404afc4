"""GPU (-m gpu): dst_group_summary / Engine.group_summary — exact against the numpy / Python-integer restatement of the
definition (group_summary_reference) applied to the context's own run_square / run_rect values, integers equal and doubles
bitwise: every measure on every kernel path, the rectangle, the group shapes, the kernels' boundaries, any slab bound,
NaN / +inf / -0.0, more than 65,535 row records, every status and the state a call leaves behind."""
import ctypes as C

import numpy as np
import pytest

import distance_amd as da
from group_summary_reference import CELL_KEYS, GROUPS_MAX, NONE, REC_KEYS, assert_group_summary, bits, check_consequences, group_summary
from helpers import CODES, LETTERS, random_alignment, uniform_codes
from test_gpu_links import datasets, interior, median

pytestmark = pytest.mark.gpu
ALL = ("n", "n_high", "raw", "jc69", "k80", "tn93")
ERR_ARG, ERR_STATE, ERR_NOMEM, ERR_CAPACITY = 1, 4, 5, 6
INF = float("inf")
# dst_group_summary.hip: kGrpWavePairs (one wave's run of a row), kGrpBlockPairs (one workgroup's), kGroupSegRows (slab rows
# per workgroup row of the column pass), kGroupFoldRecs (records per workgroup of the fold)
WAVE_PAIRS, BLOCK_PAIRS, SEG_ROWS, FOLD_RECS = 512, 2048, 64, 256


@pytest.fixture(scope="module")
def sets():
    return datasets()


def interleaved(n, groups, every=7):
    """record x in group x mod groups, every `every`-th record (from 3) in none"""
    g = np.arange(n) % groups
    if every:
        g[3::every] = -1
    return g


def same(a, b, what=""):
    assert a.keys() == b.keys(), what
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(bits(a[k]), bits(b[k])), (what, k)


def rows_before(n, r):
    """pairs of the first r rows of the square: the slab bound that ends the first slab after r rows"""
    return sum(n - 1 - i for i in range(r))


# ---- 1. every measure on every path -------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["dense", "consensus", "hybrid"])
@pytest.mark.parametrize("kind", ["low", "clade", "nrun", "uniform"])
def test_every_measure_every_path(sets, path, kind):
    codes = sets[kind]
    n = len(codes)
    part, everyone = interleaved(n, 3), interleaved(n, 3, every=0)
    upper = np.triu(np.ones((3, 3), bool))
    with da.Engine(0) as eng:
        eng.set_prep_threshold(0)
        eng.set_path(path)
        eng.upload(0, codes)
        for m in ALL:
            vals = eng.run_square(m)
            for t in (0.0, interior(vals), median(vals), INF):
                what = (path, kind, m, t)
                got = eng.group_summary(m, part, 3, t, per_record=True)
                assert_group_summary(got, group_summary(m, vals, n, n, True, t, part, 3), what)
                cells_only = eng.group_summary(m, part, 3, t)
                assert set(cells_only) == set(CELL_KEYS)
                same(cells_only, {k: got[k] for k in CELL_KEYS}, what)
                # everyone assigned: Engine.summary's totals and per-record rows, Engine.links' count
                got = eng.group_summary(m, everyone, 3, t, per_record=True)
                assert_group_summary(got, group_summary(m, vals, n, n, True, t, everyone, 3), what)
                check_consequences(got, everyone, True)
                s = eng.summary(m, t)
                for k in ("pairs", "nan_pairs", "summable_pairs", "links"):
                    assert int(got[k][upper].sum()) == s[k], (what, k)
                assert int(got["links"][upper].sum()) == eng.links(m, t, count_only=True), what
                assert np.array_equal(got["rec_within"].sum(axis=1, dtype=np.uint32), s["within"]), what
                assert np.array_equal(got["rec_summable"].sum(axis=1, dtype=np.uint32), s["summable"]), what
                # the sums as integers: every one of them is below 2^53 units here, so its double is exact
                unit = 1.0 if m in da.INT_MEASURES else 2.0 ** 37
                assert np.abs(s["sum"] * unit).max(initial=0) < 2.0 ** 53 and abs(s["total_sum"] * unit) < 2.0 ** 53
                assert np.array_equal((got["rec_sum"] * unit).sum(axis=1), s["sum"] * unit), what
                assert (got["sum"] * unit)[upper].sum() == s["total_sum"] * unit, what


# ---- 2. the rectangle -----------------------------------------------------------------------------------------------------
def test_rectangle_both_orders():
    codes = random_alignment(338, 200, seed=91)
    a, b = np.ascontiguousarray(codes[:37]), np.ascontiguousarray(codes[37:])
    with da.Engine(0) as eng:
        eng.upload(0, a)
        eng.upload(1, b)
        for rs, cs, nr, nc in ((0, 1, 37, 301), (1, 0, 301, 37)):
            rg, cg = interleaved(nr, 3), interleaved(nc, 5, every=4)
            for m in ALL:
                vals = eng.run_rect(m, rs, cs)
                for t in (0.0, interior(vals.reshape(-1)), INF):
                    got = eng.group_summary(m, rg, 3, t, square=False, row_slot=rs, col_slot=cs, col_groups=cg, n_col_groups=5,
                                            per_record=True)
                    assert got["pairs"].shape == (3, 5) and got["rec_sum"].shape == (nr, 5)
                    assert_group_summary(got, group_summary(m, vals, nr, nc, False, t, rg, 3, cg, 5), (rs, cs, m, t))
                    check_consequences(got, rg, False)
                # everyone assigned: the cells' links are Engine.links' count
                got = eng.group_summary(m, np.arange(nr) % 3, 3, 0.0, square=False, row_slot=rs, col_slot=cs,
                                        col_groups=np.arange(nc) % 5, n_col_groups=5)
                assert int(got["links"].sum()) == eng.links(m, 0.0, square=False, row_slot=rs, col_slot=cs, count_only=True)
        for s in (0, 1):
            with pytest.raises(da.DistanceError) as e:
                eng.group_summary("raw", np.zeros(len(a if s == 0 else b), int), 1, square=False, row_slot=s, col_slot=s,
                                  col_groups=np.zeros(len(a if s == 0 else b), int))
            assert e.value.status == ERR_ARG and "use the square form" in e.value.message


# ---- 3. group shapes ----------------------------------------------------------------------------------------------------
def test_group_shapes():
    n = 1030
    codes = uniform_codes(n, 64, seed=51)
    rng = np.random.default_rng(52)
    g6 = np.sort(rng.integers(0, 6, n))
    g6[rng.choice(n, 30, replace=False)] = -1
    names, order = rng.permutation(6), rng.permutation(n)
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        for m in ("n_high", "raw"):
            vals = eng.run_square(m)
            t = median(vals)
            one_group_only = np.full(n, -1)
            one_group_only[5::9] = 2
            shapes = {"G = 1": (np.zeros(n, int), 1), "an empty group": (np.zeros(n, int), 2), "empty group first": (np.ones(n, int), 2),
                      "G = DST_GROUPS_MAX": (np.arange(n) % GROUPS_MAX, GROUPS_MAX), "one group, the rest unassigned": (one_group_only, 4)}
            for name, (g, G) in shapes.items():
                got = eng.group_summary(m, g, G, t, per_record=True)
                assert_group_summary(got, group_summary(m, vals, n, n, True, t, g, G), (m, name))
            got = eng.group_summary(m, np.arange(n) % GROUPS_MAX, None, t)   # n_groups from the labels
            assert got["pairs"].shape == (GROUPS_MAX, GROUPS_MAX) and got["pairs"][0, 0] == 1 and got["pairs"][6, 6] == 0
            assert got["pairs"][0, 1] == 4 and got["pairs"][5, 6] == 2 and got["pairs"][6, 7] == 1
            # sorted labels against the same labels under other names, and against the records in another order
            base = eng.group_summary(m, g6, 6, t, per_record=True)
            assert_group_summary(base, group_summary(m, vals, n, n, True, t, g6, 6), (m, "sorted"))
            renamed = eng.group_summary(m, np.where(g6 < 0, -1, names[g6]), 6, t, per_record=True)
            for k in CELL_KEYS:
                assert np.array_equal(bits(renamed[k][np.ix_(names, names)]), bits(base[k])), (m, k)
            for k in REC_KEYS:
                assert np.array_equal(bits(renamed[k][:, names]), bits(base[k])), (m, k)
        for m, t in (("n_high", 48.0), ("raw", 0.75)):
            eng.upload(0, codes)
            base = eng.group_summary(m, g6, 6, t, per_record=True)
            eng.upload(0, np.ascontiguousarray(codes[order]))
            shuffled = eng.group_summary(m, g6[order], 6, t, per_record=True)
            same({k: shuffled[k] for k in CELL_KEYS}, {k: base[k] for k in CELL_KEYS}, (m, "shuffled"))
            for k in REC_KEYS:
                assert np.array_equal(bits(shuffled[k]), bits(base[k][order])), (m, k)


def test_every_record_its_own_group():
    n = 200
    codes = random_alignment(n, 120, seed=53, divergence=0.2)
    i, j = np.triu_indices(n, 1)
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        for m in ("n", "k80"):
            vals = eng.run_square(m)
            got = eng.group_summary(m, np.arange(n), n, median(vals), per_record=True)
            assert_group_summary(got, group_summary(m, vals, n, n, True, median(vals), np.arange(n), n), m)
            # every off-diagonal cell holds one pair, min == max == its payload (a NaN pair: the empty cell's NaN)
            assert (got["pairs"][i, j] == 1).all() and not got["pairs"][np.diag_indices(n)].any()
            # (-0.0 comes back as +0.0, a NaN pair leaves the cell without a value: the quiet NaN)
            payload = bits(vals) if m == "n" else np.where(np.isnan(vals), np.uint64(0x7FF8000000000000), bits(vals + 0.0))
            for k in ("min", "max"):
                assert np.array_equal(bits(got[k][i, j]), payload), (m, k)
                assert np.array_equal(bits(got[k]), bits(got[k].T))


# ---- 4. the kernels' boundaries ----------------------------------------------------------------------------------------
def test_row_runs_and_column_segments_square():
    """2,051 records: the rows of the square have 2,050 .. 0 entries, so they cross the 512-entry run of a wave and the
    2,048-entry run of a workgroup of the row pass one below, at and one above; slabs of 63, 64 and 65 rows end one row below,
    at and above the column pass' 64-row segment; 2,051 assigned records cross the fold's 256-record stretches."""
    n = 2051
    assert n - 1 > BLOCK_PAIRS + 1 and n > 8 * FOLD_RECS
    codes = uniform_codes(n, 64, seed=41)
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        for m, g, G in (("n_high", interleaved(n, 3), 3), ("raw", interleaved(n, 70, every=0), 70)):
            vals = eng.run_square(m)
            t = median(vals)
            want = group_summary(m, vals, n, n, True, t, g, G)
            for max_pairs in (0,) + tuple(rows_before(n, SEG_ROWS + d) for d in (-1, 0, 1)):
                assert_group_summary(eng.group_summary(m, g, G, t, max_pairs=max_pairs, per_record=True), want, (m, max_pairs))
            assert want["links"].sum() > 0 and want["rec_within"].sum() > 0


def test_row_runs_and_slabs_rectangle():
    """Rectangles whose rows have one entry below, exactly and one entry above a wave's and a workgroup's run, 66 rows cut
    into slabs of 63 / 64 / 65 rows and one."""
    codes = uniform_codes(66 + BLOCK_PAIRS + 1, 48, seed=42)
    rows, cols = np.ascontiguousarray(codes[:66]), codes[66:]
    rg = interleaved(66, 4)
    with da.Engine(0) as eng:
        eng.upload(0, rows)
        for nc in (WAVE_PAIRS - 1, WAVE_PAIRS, WAVE_PAIRS + 1, BLOCK_PAIRS - 1, BLOCK_PAIRS, BLOCK_PAIRS + 1):
            eng.upload(1, np.ascontiguousarray(cols[:nc]))
            cg = interleaved(nc, 3, every=11)
            for m in ("n", "jc69"):
                vals = eng.run_rect(m, 0, 1)
                t = median(vals.reshape(-1))
                want = group_summary(m, vals, 66, nc, False, t, rg, 4, cg, 3)
                for max_pairs in (0, 63 * nc, 64 * nc, 65 * nc, 1):
                    got = eng.group_summary(m, rg, 4, t, square=False, col_groups=cg, n_col_groups=3, max_pairs=max_pairs, per_record=True)
                    assert_group_summary(got, want, (nc, m, max_pairs))


# ---- 5. the slab bound does not change the result ----------------------------------------------------------------------
def test_slab_sizes(sets):
    codes = sets["clade"]
    n = len(codes)
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        eng.upload(1, np.ascontiguousarray(sets["low"][:41]))
        for square, nr, nc in ((True, n, n), (False, n, 41)):
            rg, cg = interleaved(nr, 5), interleaved(nc, 2)
            for m in ("n_high", "raw", "tn93"):
                vals = eng.run_square(m) if square else eng.run_rect(m, 0, 1)
                t = median(vals.reshape(-1))
                want = group_summary(m, vals, nr, nc, square, t, rg, 5, cg, 2)
                first = None
                for max_pairs in (1, 300, n - 1, n, 0):
                    got = eng.group_summary(m, rg, 5, t, square=square, col_groups=cg, n_col_groups=2, max_pairs=max_pairs, per_record=True)
                    assert_group_summary(got, want, (square, m, max_pairs))
                    first = first or got
                    same(got, first, (square, m, max_pairs))


# ---- 6. designed values ------------------------------------------------------------------------------------------------
def encode(text):
    lut = {LETTERS[k]: int(c) for k, c in enumerate(CODES)}
    return np.array([lut[c] for c in text], np.uint8)


def test_nan_pairs():
    codes = random_alignment(30, 100, seed=94)
    codes[3] = 240
    codes[7] = 240   # two records without a resolved site: every pair with one of them is 0 / 0
    g = np.arange(30) % 2
    g[3] = 2         # one in a group of its own, the other (7) shares group 1
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        vals = eng.run_square("raw")
        assert np.isnan(vals).sum() == 2 * 28 + 1
        for t in (0.0, 0.5, INF):
            got = eng.group_summary("raw", g, 3, t, per_record=True)
            assert_group_summary(got, group_summary("raw", vals, 30, 30, True, t, g, 3), t)
        assert got["pairs"][2].tolist() == [15, 14, 0] and got["nan_pairs"][2].tolist() == [15, 14, 0]
        assert np.isnan(got["min"][2]).all() and np.isnan(got["max"][2]).all() and not got["sum"][2].any()
        assert bits(got["min"][2]).tolist() == [0x7FF8000000000000] * 3
        assert got["nan_pairs"][1, 1] == 13 and got["summable_pairs"][1, 1] == 14 * 13 // 2 - 13 and np.isfinite(got["min"][1, 1])
        assert not got["rec_summable"][3].any() and not got["rec_summable"][7].any()


def test_negative_zero_and_infinity():
    a = b"ACGTACGTACGTACGTAAAA"
    rows = [a, a, b"CATGCATGCATGCATTAAAA",    # 15 of 20 sites differ from a: p = 0.75, jc69 +inf
            b"GTACGTACGTGTACGTAAAA",          # 10 of 20 sites are transitions of a: P = 0.5, Q = 0, k80 +inf
            b"CATGCATGCATGCATGAAAA"]          # p = 0.8: NaN
    codes = np.stack([encode(r) for r in rows])
    g = np.array([0, 0, 1, 1, 1])
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        for m in ("jc69", "k80"):
            vals = eng.run_square(m)
            assert vals[0] == 0.0 and np.signbit(vals[0]), m   # the pair (0, 1): -0.0
            assert np.isposinf(vals).any() and np.isnan(vals).any()
            for t in (0.0, -0.0, 1e308, INF):
                got = eng.group_summary(m, g, 2, t, per_record=True)
                assert_group_summary(got, group_summary(m, vals, 5, 5, True, t, g, 2), (m, t))
            assert bits(got["min"])[0, 0] == 0 and bits(got["max"])[0, 0] == 0   # -0.0 is reported as +0.0
            assert got["links"][0, 0] == 1 and np.isposinf(got["max"]).any() and np.isfinite(got["sum"]).all()
            assert eng.group_summary(m, g, 2, 0.0)["links"][0, 0] == 1            # -0.0 links at T = 0.0


def test_thresholds_of_the_integer_measures(sets):
    codes = sets["uniform"]
    n = len(codes)
    g = interleaved(n, 3)
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        for m in ("n", "n_high"):
            vals = eng.run_square(m)
            for t in (-1e30, -2.0 ** 63, -1.0, 2.0 ** 63, 1e30, INF, -INF):
                got = eng.group_summary(m, g, 3, t, per_record=True)
                assert_group_summary(got, group_summary(m, vals, n, n, True, t, g, 3), (m, t))
                if t < -2.0 ** 63 or t == -1.0:
                    assert not got["links"].any() and not got["rec_within"].any()
                if t >= 2.0 ** 63:
                    assert np.array_equal(got["links"], got["pairs"])


# ---- 7. more than 65,535 row records -------------------------------------------------------------------------------------
def test_two_row_grids():
    """65,537 row records against 5: launch_group_rows gives every row a grid row (for_row_grids), so the row pass takes
    two grids of at most 65,535 rows; the fold walks 65,537 assigned records."""
    nr = 65537
    codes = uniform_codes(nr + 5, 16, seed=42)
    rg = interleaved(nr, 4, every=0)
    cg = np.array([0, 1, 0, -1, 1])
    with da.Engine(0) as eng:
        eng.upload(0, np.ascontiguousarray(codes[:nr]))
        eng.upload(1, np.ascontiguousarray(codes[nr:]))
        for m in ("n", "jc69"):
            vals = eng.run_rect(m, 0, 1)
            t = median(vals.reshape(-1))
            got = eng.group_summary(m, rg, 4, t, square=False, col_groups=cg, n_col_groups=2, per_record=True)
            assert_group_summary(got, group_summary(m, vals, nr, 5, False, t, rg, 4, cg, 2), m)
            if m == "n":
                assert got["rec_summable"][65535:].tolist() == [[2, 2], [2, 2]]   # (the second grid's rows count)


# ---- 8. statuses, trivial shapes, state -------------------------------------------------------------------------------
def test_errors():
    """Every status that a test-sized call can reach.  Not reached: DST_ERR_NOMEM (the state of 1,024 groups fits any set
    the suite can upload) and the 2^32 - 1 records check (two_sets' own, shared with dst_summary)."""
    lib = da.load()
    codes = random_alignment(50, 100, seed=96)
    cells = (da._lib.GroupCell * 16)()
    rw, rs_, rsum = np.full(200, 7, np.uint32), np.full(200, 7, np.uint32), np.full(200, 7.0)
    labels = (np.arange(50) % 4).astype(np.uint32)
    col_labels = (np.arange(5) % 2).astype(np.uint32)

    def call(h, m=2, square=1, rs=0, cs=1, rg=labels, Gr=4, cg=None, Gc=2, t=1.0, cp=C.addressof(cells), ccap=16, rec=True, rcap=200):
        return lib.dst_group_summary(h, m, square, rs, cs, None if rg is None else rg.ctypes.data, Gr,
                                     None if cg is None else cg.ctypes.data, Gc, t, 0, cp, ccap, rw.ctypes.data if rec else None,
                                     rs_.ctypes.data if rec else None, rsum.ctypes.data if rec else None, rcap)

    def message(h):
        return lib.dst_last_error(h)

    assert call(None) == ERR_ARG
    with da.Engine(0) as eng:
        h = eng._h
        assert call(h) == ERR_STATE and b"not uploaded" in message(h)
        eng.upload(0, codes)
        assert call(h, square=0, cg=col_labels) == ERR_STATE   # slot 1 is empty
        assert call(h, rg=None) == ERR_ARG and call(h, cp=None, rec=False) == ERR_ARG
        assert call(h, square=0) == ERR_ARG and b"col_group" in message(h)
        assert call(h, m=9) == ERR_ARG and call(h, m=-1) == ERR_ARG and b"unknown measure" in message(h)
        assert call(h, t=float("nan")) == ERR_ARG and b"threshold is NaN" in message(h)
        assert call(h, square=0, cg=col_labels, rs=2) == ERR_ARG and call(h, square=0, cg=col_labels, cs=-1) == ERR_ARG
        assert call(h, square=0, cg=col_labels, rs=1, cs=1) == ERR_ARG and b"use the square form" in message(h)
        assert call(h, Gr=0) == ERR_ARG and call(h, Gr=GROUPS_MAX + 1) == ERR_ARG
        bad = labels.copy()
        bad[17] = 4
        bad[30] = 9
        assert call(h, rg=bad) == ERR_ARG and b"record 17" in message(h) and b"label 4" in message(h) and b"set" in message(h)
        bad[17] = NONE
        assert call(h, rg=bad) == ERR_ARG and b"record 30" in message(h)
        assert call(h, ccap=15) == ERR_CAPACITY and b"cells_cap" in message(h) and b"16" in message(h)
        assert call(h, rcap=199) == ERR_CAPACITY and b"rec_cap" in message(h) and b"200" in message(h)
        assert call(h, rcap=0, rec=False) == 0 and call(h, cp=None, ccap=0) == 0
        eng.upload(1, random_alignment(5, 90, seed=97))
        assert call(h, square=0, cg=col_labels) == ERR_STATE and b"Different length sequences" in message(h)
        eng.upload(1, random_alignment(5, 100, seed=97))
        assert call(h, square=0, cg=col_labels, Gc=0) == ERR_ARG and call(h, square=0, cg=col_labels, Gc=GROUPS_MAX + 1) == ERR_ARG
        bad_col = col_labels.copy()
        bad_col[3] = 2
        assert call(h, square=0, cg=bad_col) == ERR_ARG and b"column record 3" in message(h)
        assert call(h, square=0, rg=bad, cg=col_labels) == ERR_ARG and b"row record 30" in message(h)
        assert call(h, square=0, cg=col_labels, ccap=7) == ERR_CAPACITY and call(h, square=0, cg=col_labels, rcap=99) == ERR_CAPACITY
        assert call(h, square=0, cg=col_labels, ccap=8, rcap=100) == 0
        assert call(h, t=INF) == 0 and sum(cells[4 * a + b].pairs for a in range(4) for b in range(a, 4)) == 50 * 49 // 2
        assert int(rw[:200].sum()) == 50 * 49   # threshold inf: every partner of every record is within


def test_trivial_shapes():
    codes = random_alignment(4, 50, seed=95, divergence=0.3)
    with da.Engine(0) as eng:
        eng.upload(0, codes[:1])
        for m in ("n", "raw"):
            got = eng.group_summary(m, [0], 2, INF, per_record=True)
            for k in CELL_KEYS[:5] + REC_KEYS:
                assert not got[k].any(), (m, k)
            assert got["rec_sum"].shape == (1, 2)
            assert bits(got["min"]).tolist() == bits(got["max"]).tolist() == [[0 if m == "n" else 0x7FF8000000000000] * 2] * 2
        eng.upload(0, codes)
        eng.upload(1, codes[:2])
        before = eng.run_square("raw")
        for m in ("n", "raw"):
            # no record assigned: nothing in any cell, nothing in any row
            got = eng.group_summary(m, [-1] * 4, 3, INF, per_record=True)
            assert all(not got[k].any() for k in CELL_KEYS[:5] + REC_KEYS) and got["pairs"].shape == (3, 3)
            got = eng.group_summary(m, [0, 1, 0, 1], 2, INF, square=False, col_groups=[NONE, NONE], n_col_groups=3, per_record=True)
            assert all(not got[k].any() for k in CELL_KEYS[:5] + REC_KEYS) and got["rec_within"].shape == (4, 3)
            # no ROW record assigned: the cells are empty, the rows are not
            vals = eng.run_rect(m, 0, 1)
            got = eng.group_summary(m, [-1] * 4, 2, INF, square=False, col_groups=[1, 0], n_col_groups=2, per_record=True)
            assert_group_summary(got, group_summary(m, vals, 4, 2, False, INF, [-1] * 4, 2, [1, 0], 2), m)
            assert not got["pairs"].any() and got["rec_summable"].all()
            assert not eng.group_summary(m, [-1] * 4, 2, INF, square=False, col_groups=[1, 0], n_col_groups=2)["pairs"].any()
        assert np.array_equal(bits(eng.run_square("raw")), bits(before))
        # two records, one pair
        eng.upload(0, np.ascontiguousarray(codes[[0, 0]]))
        got = eng.group_summary("raw", [1, 0], 2, 0.0, per_record=True)
        assert got["pairs"].tolist() == [[0, 1], [1, 0]] and got["links"].tolist() == [[0, 1], [1, 0]]
        assert got["rec_within"].tolist() == [[1, 0], [0, 1]]


@pytest.mark.parametrize("path", ["auto", "dense", "consensus"])
def test_state_unchanged(sets, path):
    codes = sets["nrun"]
    n = len(codes)
    g = interleaved(n, 3)
    with da.Engine(0) as eng:
        eng.set_prep_threshold(0)
        eng.set_path(path)
        eng.upload(0, codes)
        eng.upload(1, np.ascontiguousarray(sets["low"][:20]))
        for m in ("raw", "tn93"):
            before = eng.run_square(m)
            used = eng.last_path()
            summary_before = eng.summary(m, interior(before), bins=16, width=0.01)
            calls = (lambda: eng.group_summary(m, g, 3, interior(before), max_pairs=2000, per_record=True),
                     lambda: eng.group_summary(m, g, 3, interior(before)),
                     lambda: eng.group_summary(m, g, 3, 0.0, square=False, col_groups=interleaved(20, 2), n_col_groups=2, per_record=True))
            for call in calls:
                first = call()
                same(call(), first, (path, m))   # a second identical call: identical bytes
                after = eng.run_square(m)
                assert np.array_equal(bits(before), bits(after)) and eng.last_path() == used, (path, m)
                again = eng.summary(m, interior(before), bins=16, width=0.01)
                same({k: np.asarray(v) for k, v in again.items()}, {k: np.asarray(v) for k, v in summary_before.items()}, (path, m))


def test_between_the_other_analyses(sets):
    """The slab scratch is shared: group summaries before and after clusters, nearest and summary on one context, each
    result that of the first call."""
    codes = sets["clade"]
    g = interleaved(len(codes), 4)
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        first = {m: eng.group_summary(m, g, 4, t, per_record=True) for m, t in (("tn93", 0.002), ("n_high", 3.0))}
        for other in (lambda: eng.clusters("n_high", 3.0, max_pairs=500), lambda: eng.nearest("tn93", k=3, tallies=True),
                      lambda: eng.summary("raw", 0.01, bins=32, width=0.001, max_pairs=700)):
            other()
            same(eng.group_summary("tn93", g, 4, 0.002, max_pairs=700, per_record=True), first["tn93"])
            same(eng.group_summary("n_high", g, 4, 3.0, per_record=True), first["n_high"])
