"""GPU (-m gpu): dst_run_pairs against run_square / run_rect indexed at the canonical position, bitwise (f64 as uint64, so
NaNs compare), for every measure and both routes: the table of all code pairs, the chunk and lane-group edges, the wide
tallies, the paths, the batch and slab bounds, caller-supplied tn93 base counts, and the errors."""
import ctypes as C

import numpy as np
import pytest

import distance_amd as da
import oracle
from helpers import CODES, KNOWN, uniform_codes
from tools import synth

pytestmark = pytest.mark.gpu
ALL = ("n", "n_high", "raw", "jc69", "k80", "tn93")
ROUTES = ("direct", "sweep")
ERR_ARG, ERR_STATE, ERR_CAPACITY = 1, 4, 6
LENGTHS = (1, 127, 128, 129, 257, 513, 1025, 2049, 4097, 8191, 8192, 8193)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same(got_v, got_t, want_v, want_t, what):
    assert got_v.dtype == want_v.dtype and np.array_equal(bits(got_v), bits(want_v)), (what, "values")
    assert got_t.dtype == np.uint32 and np.array_equal(got_t, want_t), (what, "tallies")


def square_reference(eng, m, n, row, col):
    """values and tallies of the listed pairs from run_square at the canonical position; the diagonal from run_rect of
    slot 0 against the same set in slot 1 (which the caller has uploaded when the list holds a diagonal entry)"""
    row, col = np.asarray(row, np.int64), np.asarray(col, np.int64)
    lo, hi = np.minimum(row, col), np.maximum(row, col)
    diag = lo == hi
    at = np.where(diag, 0, lo * (2 * n - lo - 1) // 2 + (hi - lo - 1))
    width = da.tally_width(m)
    v = eng.run_square(m)
    t = eng.run_square(m, tallies=True).reshape(-1, width)
    if v.size == 0:   # (one record: nothing but the diagonal)
        v, t = np.zeros(1, v.dtype), np.zeros((1, width), np.uint32)
    want_v, want_t = v[at].copy(), t[at].copy()
    if diag.any():
        rv = eng.run_rect(m, 0, 1)
        rt = eng.run_rect(m, 0, 1, tallies=True).reshape(n, n, width)
        want_v[diag], want_t[diag] = rv[lo[diag], lo[diag]], rt[lo[diag], lo[diag]]
    return want_v, want_t


def check_square(eng, m, n, row, col, routes=ROUTES, **kw):
    want_v, want_t = square_reference(eng, m, n, row, col)
    infos = {}
    for route in routes:
        got_v, got_t, infos[route] = eng.run_pairs(m, row, col, values=True, tallies=True, route=route, info=True, **kw)
        same(got_v, got_t, want_v, want_t, (m, route, "both"))
        # (each output alone: the sweep then runs its slabs in the other output kind)
        assert np.array_equal(bits(eng.run_pairs(m, row, col, route=route, **kw)), bits(want_v)), (m, route, "values alone")
        assert np.array_equal(eng.run_pairs(m, row, col, values=False, tallies=True, route=route, **kw), want_t), (m, route)
    return infos


def check_rect(eng, m, row, col, row_slot, col_slot, routes=ROUTES, **kw):
    n_rows, n_cols = eng.set_info(row_slot)[0], eng.set_info(col_slot)[0]
    width = da.tally_width(m)
    want_v = eng.run_rect(m, row_slot, col_slot)[row, col]
    want_t = eng.run_rect(m, row_slot, col_slot, tallies=True).reshape(n_rows, n_cols, width)[row, col]
    for route in routes:
        got_v, got_t = eng.run_pairs(m, row, col, square=False, row_slot=row_slot, col_slot=col_slot, values=True, tallies=True,
                                     route=route, **kw)
        same(got_v, got_t, want_v, want_t, (m, route, "rect", row_slot))


def test_code_table():
    """17 records of one code each against one record of all 17 codes: every (a, b), both ways, and as a square of all 18 with
    its diagonal, whose tallies are the oracle's per-site table summed over the record against itself"""
    table = np.repeat(CODES[:, None], 17, axis=1)
    one = CODES[None, :].copy()
    both = np.concatenate([table, one])
    r17, z17 = np.arange(17), np.zeros(17, np.int64)
    sq_row, sq_col = [x.ravel() for x in np.meshgrid(np.arange(18), np.arange(18), indexing="ij")]
    with da.Engine(0) as eng:
        eng.upload(0, table)
        eng.upload(1, one)
        for m in ALL:
            check_rect(eng, m, r17, z17, 0, 1)
            check_rect(eng, m, z17, r17, 1, 0)
        eng.upload(0, both)
        eng.upload(1, both)
        for m in ALL:
            check_square(eng, m, 18, sq_row, sq_col)
            _, tal = eng.run_pairs(m, np.arange(18), np.arange(18), values=True, tallies=True, route="sweep")
            want = np.array([oracle.tallies(m, both[i], both[i]) for i in range(18)])
            assert np.array_equal(tal.astype(np.int64), want.astype(np.int64).reshape(18, -1)), m


def edge_sets(n, length):
    rng = np.random.default_rng(1000 * n + length)
    codes = uniform_codes(n, length, seed=n + length)
    codes[:, rng.random(length) < 0.5] = 136          # (half the columns agree, so that pairs differ in their values)
    other = uniform_codes(3, length, seed=7 * n + length)
    forced = sorted({s for s in (0, 127, 128, length - 1) if s < length})
    codes[0, forced], codes[1, forced], other[2, forced] = 136, 40, 24
    if n <= 65:
        row, col = [x.ravel() for x in np.meshgrid(np.arange(n), np.arange(n), indexing="ij")]   # i < j, i > j, i == j
    else:
        row, col = rng.integers(0, n, 600), rng.integers(0, n, 600)
    row = np.concatenate([[1, 0, 1, n - 1, 0], row, [0, 1]])   # unsorted, with repeats
    col = np.concatenate([[0, 1, 1, 0, 1], col, [1, 0]])
    r_row, r_col = rng.integers(0, n, 50), rng.integers(0, 3, 50)
    r_row[0], r_col[0] = 0, 2
    return codes, other, row, col, r_row, r_col


@pytest.mark.parametrize("n", [2, 3, 65, 257])
@pytest.mark.parametrize("length", LENGTHS)
def test_chunk_edges(n, length):
    codes, other, row, col, r_row, r_col = edge_sets(n, length)
    lanes = int(da.load().dst_run_pairs_lanes(length))
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        eng.upload(1, other)
        for m in ALL:
            check_rect(eng, m, r_row, r_col, 0, 1)
        eng.upload(1, codes)
        for m in ALL:
            infos = check_square(eng, m, n, row, col)
            assert infos["direct"]["route"] == "direct" and infos["direct"]["lanes_per_pair"] == lanes
            assert infos["direct"]["direct_pairs"] == row.size and infos["direct"]["slabs"] == 0
            n_diag = int((row == col).sum())
            assert infos["sweep"]["route"] == "sweep" and infos["sweep"]["direct_pairs"] == n_diag
            assert infos["sweep"]["swept_pairs"] == row.size - n_diag and infos["sweep"]["slabs"] == 1
            assert infos["sweep"]["lanes_per_pair"] == lanes   # (the diagonal entries' launch)
            got = eng.run_pairs(m, [], [], values=True, tallies=True, route="direct", info=True)
            assert got[0].size == 0 and got[1].shape == (0, da.tally_width(m)) and got[2]["lanes_per_pair"] == 0


def test_lane_groups():
    """the lengths of test_chunk_edges reach every lane-group size the launcher can choose, and the wrap past 64 chunks"""
    lib = da.load()
    every = {int(lib.dst_run_pairs_lanes(length)) for length in range(0, 70 * 128, 64)}
    assert every == {1, 2, 4, 8, 16, 32, 64}
    reached = set()
    for length in LENGTHS:
        codes, _, row, col, _, _ = edge_sets(3, length)
        with da.Engine(0) as eng:
            eng.upload(0, codes)
            eng.upload(1, codes)
            infos = check_square(eng, "tn93", 3, row, col, routes=("direct",))
            assert infos["direct"]["lanes_per_pair"] == int(lib.dst_run_pairs_lanes(length))
            reached.add(infos["direct"]["lanes_per_pair"])
    assert reached == every
    assert (max(LENGTHS) + 127) // 128 > 64


@pytest.mark.parametrize("consensus", [False, True])
def test_wide_tallies(consensus):
    """65,537 sites that all differ: one more than a 16-bit tally holds, on the sweep's kernels and in the direct kernel"""
    length = 65537
    codes = np.empty((3, length), np.uint8)
    codes[0], codes[1], codes[2] = 136, 40, 24
    codes[2, :5] = 136
    row, col = [x.ravel() for x in np.meshgrid(np.arange(3), np.arange(3), indexing="ij")]
    with da.Engine(0) as eng:
        if consensus:
            eng.set_prep_threshold(0)
            eng.set_path("consensus")
        eng.upload(0, codes)
        eng.upload(1, codes)
        for m in ALL:
            check_square(eng, m, 3, row, col)
        tal = eng.run_pairs("n", [0], [1], values=False, tallies=True, route="direct")
        assert tal.tolist() == [[length]]


def test_paths():
    """the same set on a dense context and on one whose upload deferred the planes: identical results; only the direct route
    asks for the planes; the caller's last launch and later runs are untouched"""
    n, length = 1100, 3333
    rng = np.random.default_rng(31)
    codes = synth.alignment(synth.SEED ^ 31, n, length)
    for r in rng.choice(n, 50, replace=False):
        at = rng.choice(length, 20, replace=False)
        codes[r, at] = CODES[rng.integers(0, 17, len(at))]
    row, col = rng.integers(0, n, 5000), rng.integers(0, n, 5000)
    keep = row != col
    row, col = row[keep], col[keep]
    with da.Engine(0) as dense, da.Engine(0) as lazy:
        dense.set_path("dense")
        dense.upload(0, codes)
        assert dense.planes_stored(0)
        lazy.set_prep_threshold(0)
        lazy.upload(0, codes)
        assert not lazy.planes_stored(0), "the upload stored every plane: nothing here tests the deferred form"
        lazy.set_path("consensus")   # (the path that never asks for planes)
        before = {m: lazy.run_square(m) for m in ("n", "tn93")}
        assert not lazy.planes_stored(0) and lazy.last_path() == "consensus"
        first = True
        for m in ALL:
            want_v, want_t = square_reference(dense, m, n, row, col)
            got = lazy.run_pairs(m, row, col, values=True, tallies=True, route="sweep")
            same(got[0], got[1], want_v, want_t, (m, "deferred", "sweep"))
            if first:
                assert not lazy.planes_stored(0), "the sweep route asked for the planes of a consensus-path context"
            launch, path = repr(lazy.last_launch()), lazy.last_path()
            got = lazy.run_pairs(m, row, col, values=True, tallies=True, route="direct")
            same(got[0], got[1], want_v, want_t, (m, "deferred", "direct"))
            assert lazy.planes_stored(0)
            assert repr(lazy.last_launch()) == launch and lazy.last_path() == path
            first = False
            launch, path = repr(dense.last_launch()), dense.last_path()
            for route in ROUTES:
                got = dense.run_pairs(m, row, col, values=True, tallies=True, route=route)
                same(got[0], got[1], want_v, want_t, (m, "dense", route))
                assert repr(dense.last_launch()) == launch and dense.last_path() == path
        for m, v in before.items():
            assert lazy.run_square(m).tobytes() == v.tobytes() and lazy.last_path() == "consensus", m
            assert np.array_equal(dense.run_square(m), v, equal_nan=True), m


def test_batch_bound():
    """one pair more than a device batch, on 5 records of 130 sites"""
    n, length = 5, 130
    rng = np.random.default_rng(51)
    codes = uniform_codes(n, length, seed=51)
    count = da.RUN_PAIRS_BATCH + 1
    row, col = rng.integers(0, n, count), rng.integers(0, n, count)
    row[-1], col[-1] = 4, 0   # (the entry of the second batch)
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        eng.upload(1, codes)
        for m in ("n", "tn93"):
            want_v, want_t = square_reference(eng, m, n, row, col)
            got_v, got_t, info = eng.run_pairs(m, row, col, values=True, tallies=True, route="direct", info=True)
            same(got_v, got_t, want_v, want_t, m)
            assert info["direct_pairs"] == count and info["lanes_per_pair"] == 2
            got_v, got_t = eng.run_pairs(m, row, col, values=True, tallies=True, route="sweep")
            same(got_v, got_t, want_v, want_t, (m, "sweep"))


def test_slab_bounds():
    """single-row slabs on 65 records; a list that touches the last slab only; auto agrees with both routes"""
    n, length = 65, 300
    rng = np.random.default_rng(61)
    codes = uniform_codes(n, length, seed=61)
    codes[:, rng.random(length) < 0.6] = 72
    row, col = rng.integers(0, n, 900), rng.integers(0, n, 900)
    off = row != col
    rows_hit = len(set(np.minimum(row, col)[off].tolist()))
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        eng.upload(1, codes)
        for m in ALL:
            infos = check_square(eng, m, n, row, col, max_pairs=1)
            assert infos["sweep"]["slabs"] == rows_hit and infos["direct"]["slabs"] == 0
            want_v, want_t = square_reference(eng, m, n, row, col)
            for max_pairs in (0, 1, 100):
                got_v, got_t, info = eng.run_pairs(m, row, col, values=True, tallies=True, route="auto", max_pairs=max_pairs,
                                                   info=True)
                same(got_v, got_t, want_v, want_t, (m, "auto", max_pairs))
                assert info["route"] in ROUTES
            last_row, last_col = np.array([n - 1, n - 2, n - 2]), np.array([n - 2, n - 1, n - 1])
            infos = check_square(eng, m, n, last_row, last_col, max_pairs=1)
            assert infos["sweep"]["slabs"] == 1 and infos["sweep"]["swept_pairs"] == 3
        # a rectangle in single-row slabs
        eng.upload(1, uniform_codes(7, length, seed=62))
        r_row, r_col = rng.integers(0, n, 200), rng.integers(0, 7, 200)
        for m in ALL:
            check_rect(eng, m, r_row, r_col, 0, 1, max_pairs=7)
            check_rect(eng, m, r_col, r_row, 1, 0, max_pairs=1)


def test_tn93_supplied_counts():
    """base counts the caller uploaded, different from the counts by code: the values follow run_square's, (j, i) is (i, j)"""
    n, length = 40, 500
    rng = np.random.default_rng(71)
    codes = np.array(KNOWN, np.uint8)[rng.integers(0, 4, (n, length))]
    codes[:, rng.random(length) < 0.8] = 136
    counts = rng.integers(1, 400, (n, 4)).astype(np.uint32)
    row, col = [x.ravel() for x in np.meshgrid(np.arange(n), np.arange(n), indexing="ij")]
    off = row != col
    row, col = row[off], col[off]
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        by_code = eng.run_square("tn93")
        eng.upload(0, codes, counts)
        assert not np.array_equal(bits(eng.run_square("tn93")), bits(by_code)), "the supplied counts change nothing: no test"
        want_v, want_t = square_reference(eng, "tn93", n, row, col)
        for route in ROUTES:
            got_v, got_t = eng.run_pairs("tn93", row, col, values=True, tallies=True, route=route)
            same(got_v, got_t, want_v, want_t, route)
            back = eng.run_pairs("tn93", col, row, route=route)
            assert np.array_equal(bits(back), bits(got_v)), route


def test_errors():
    codes = uniform_codes(9, 200, seed=5)
    lib = da.load()
    with da.Engine(0) as eng:
        h = eng._h
        with pytest.raises(da.DistanceError) as e:
            eng.run_pairs("raw", [0, 1], [1, 0])
        assert e.value.status == ERR_STATE
        eng.upload(0, codes)
        for route in ROUTES + ("auto",):
            with pytest.raises(da.DistanceError) as e:
                eng.run_pairs("raw", [0, 3, 9, 12], [1, 2, 0, 0], route=route)
            assert e.value.status == ERR_ARG and "pair 2 " in e.value.message
        with pytest.raises(da.DistanceError) as e:
            eng.run_pairs("raw", [0, 3], [1, 9])
        assert e.value.status == ERR_ARG and "pair 1 " in e.value.message
        for s in (0, 1):
            with pytest.raises(da.DistanceError) as e:
                eng.run_pairs("raw", [0], [1], square=False, row_slot=s, col_slot=s)
            assert e.value.status == ERR_ARG
        with pytest.raises(da.DistanceError) as e:
            eng.run_pairs("raw", [0], [0], square=False, row_slot=0, col_slot=1)
        assert e.value.status == ERR_STATE   # (slot 1 is not uploaded)
        with pytest.raises(da.DistanceError) as e:
            eng.run_pairs("raw", [0], [1], route=7)
        assert e.value.status == ERR_ARG and "route" in e.value.message
        row, col = np.array([0, 5, 2, 2], np.uint32), np.array([8, 1, 2, 7], np.uint32)

        def call(measure=2, r=row, c=col, values=True, tallies=True, cap=row.size, route=1):
            v, t = np.full(row.size, 77, np.uint64), np.full((row.size, 2), 77, np.uint32)
            rc = lib.dst_run_pairs(h, measure, 1, 0, 1, None if r is None else r.ctypes.data, None if c is None else c.ctypes.data,
                                   row.size, route, 0, v.ctypes.data if values else None, t.ctypes.data if tallies else None, cap,
                                   None)
            return rc, v, t

        rc, v, t = call()
        assert rc == 0 and not (v == 77).any() and not (t == 77).all()
        rc, v, t = call(cap=row.size - 1)
        assert rc == ERR_CAPACITY and (v == 77).all() and (t == 77).all()
        assert call(values=False, tallies=False)[0] == ERR_ARG
        assert call(values=False)[0] == 0 and call(tallies=False)[0] == 0
        assert call(r=None)[0] == ERR_ARG and call(c=None)[0] == ERR_ARG
        assert call(measure=6)[0] == ERR_ARG and call(measure=-1)[0] == ERR_ARG
        assert call(route=3)[0] == ERR_ARG and call(route=-1)[0] == ERR_ARG
        assert lib.dst_run_pairs(None, 2, 1, 0, 1, row.ctypes.data, col.ctypes.data, row.size, 1, 0, v.ctypes.data, None, row.size,
                                 None) == ERR_ARG
        eng.upload(1, uniform_codes(5, 90, seed=6))
        with pytest.raises(da.DistanceError) as e:
            eng.run_pairs("raw", [0], [0], square=False, row_slot=0, col_slot=1)
        assert e.value.status == ERR_STATE and "Different length sequences" in e.value.message
        eng.upload(1, codes)
        check_square(eng, "raw", 9, row, col)
