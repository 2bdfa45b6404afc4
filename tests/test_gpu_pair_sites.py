"""GPU (-m gpu): dst_pair_sites against the numpy restatement of its definition (pair_sites_reference): the table of all
code pairs, the chunk edges, the paths, the batch and window bounds, one pair longer than a window, and the errors."""
import ctypes as C

import numpy as np
import pytest

import distance_amd as da
from helpers import CODES, KNOWN, uniform_codes
from pair_sites_reference import DIFF_WORDS, expected
from tools import synth

pytestmark = pytest.mark.gpu
ALL = ("n", "n_high", "raw", "jc69", "k80", "tn93")
ERR_ARG, ERR_STATE, ERR_CAPACITY = 1, 4, 6


def assert_csr(got, want, what):
    for g, w, name in zip(got, want, ("offsets", "sites", "bases")):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, name)


def test_code_table():
    """17 records of one code each against one record of all 17 codes: every (a, b), both ways, and as a square of all 18"""
    table = np.repeat(CODES[:, None], 17, axis=1)
    one = CODES[None, :].copy()
    both = np.concatenate([table, one])
    r17, z17 = np.arange(17), np.zeros(17, np.int64)
    sq_row, sq_col = [x.ravel() for x in np.meshgrid(np.arange(18), np.arange(18), indexing="ij")]
    with da.Engine(0) as eng:
        eng.upload(0, table)
        eng.upload(1, one)
        for m in ALL:
            assert_csr(eng.pair_sites(m, r17, z17, square=False, row_slot=0, col_slot=1), expected(m, table, one, r17, z17), m)
            assert_csr(eng.pair_sites(m, z17, r17, square=False, row_slot=1, col_slot=0), expected(m, one, table, z17, r17), m)
        eng.upload(0, both)
        for m in ALL:
            want = expected(m, both, both, sq_row, sq_col)
            assert_csr(eng.pair_sites(m, sq_row, sq_col), want, m)
            assert int(want[0][-1]) > 0


def canonical_tally(tal, n, i, j):
    """the DST_OUT_TALLY words of the square's pair {i, j}; zeros for i == j"""
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    at = lo * (2 * n - lo - 1) // 2 + (hi - lo - 1)
    out = tal[np.where(lo == hi, 0, at)]
    out[lo == hi] = 0
    return out


@pytest.mark.parametrize("n", [2, 3, 65, 257])
@pytest.mark.parametrize("length", [1, 127, 128, 129, 256, 257, 1000])
def test_chunk_edges(n, length):
    rng = np.random.default_rng(1000 * n + length)
    codes = uniform_codes(n, length, seed=n + length)
    codes[:, rng.random(length) < 0.5] = 136          # (half the columns agree, so that pairs differ in their counts)
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
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        eng.upload(1, other)
        for m in ALL:
            want = expected(m, codes, codes, row, col)
            got = eng.pair_sites(m, row, col)
            assert_csr(got, want, m)
            assert np.array_equal(eng.pair_sites(m, row, col, count_only=True), want[0])
            tal = eng.run_square(m, tallies=True).reshape(n * (n - 1) // 2, -1).astype(np.int64)
            diff = canonical_tally(tal, n, row, col)[:, DIFF_WORDS[m]].sum(axis=1)
            assert np.array_equal(np.diff(got[0].astype(np.int64)), diff), m
            if m in ("n", "raw", "k80"):
                assert int(got[0][2]) - int(got[0][1]) >= (len(forced) if m != "k80" else 0)   # pair (0, 1): the forced sites
                assert got[1].size == 0 or int(got[1].max()) < length
            want = expected(m, codes, other, r_row, r_col)
            got = eng.pair_sites(m, r_row, r_col, square=False, row_slot=0, col_slot=1)
            assert_csr(got, want, (m, "rect"))
            tal = eng.run_rect(m, 0, 1, tallies=True).reshape(n, 3, -1).astype(np.int64)
            assert np.array_equal(np.diff(got[0].astype(np.int64)), tal[r_row, r_col][:, DIFF_WORDS[m]].sum(axis=1)), m
            got = eng.pair_sites(m, [], [])
            assert got[0].tolist() == [0] and got[1].size == 0 and got[2].size == 0


def test_paths():
    """the same set on a dense context and on one whose upload deferred the planes: identical results, later runs untouched"""
    n, length = 1100, 3333
    rng = np.random.default_rng(31)
    codes = synth.alignment(synth.SEED ^ 31, n, length)
    for r in rng.choice(n, 50, replace=False):
        at = rng.choice(length, 20, replace=False)
        codes[r, at] = CODES[rng.integers(0, 17, len(at))]
    row, col = rng.integers(0, n, 5000), rng.integers(0, n, 5000)
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
        for m in ALL:
            want = expected(m, codes, codes, row, col)
            assert_csr(dense.pair_sites(m, row, col), want, (m, "dense"))
            assert_csr(lazy.pair_sites(m, row, col), want, (m, "deferred"))
            assert lazy.planes_stored(0)
        for m, v in before.items():
            assert lazy.run_square(m).tobytes() == v.tobytes() and lazy.last_path() == "consensus", m
            assert np.array_equal(dense.run_square(m), v, equal_nan=True), m


def test_batch_and_window_bounds():
    """1,124,250 pairs (more than a batch) of about 30 entries each: the first batch alone passes the window"""
    n, length = 1500, 40
    rng = np.random.default_rng(41)
    codes = np.array(KNOWN, np.uint8)[rng.integers(0, 4, (n, length))]
    row, col = np.triu_indices(n, 1)
    assert row.size == 1_124_250 > da.PAIR_SITES_BATCH
    want = expected("raw", codes, codes, row, col)
    assert int(want[0][da.PAIR_SITES_BATCH]) > da.PAIR_SITES_WINDOW
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        assert np.array_equal(eng.pair_sites("raw", row, col, count_only=True), want[0])
        assert_csr(eng.pair_sites("raw", row, col), want, "raw")


def test_one_long_pair():
    """one pair of 2^24 + 1 entries: it straddles a window, over more than 131,072 chunks"""
    length = (1 << 24) + 1
    codes = np.empty((2, length), np.uint8)
    codes[0], codes[1] = 136, 40
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        off, sites, bases = eng.pair_sites("n", [0], [1])
        assert off.tolist() == [0, length]
        assert np.array_equal(sites, np.arange(length, dtype=np.uint32))
        assert bases.size == length and bool((bases == 0x82).all())
        off, sites, bases = eng.pair_sites("tn93", [1, 0], [0, 0])
        assert off.tolist() == [0, length, length] and int(sites[-1]) == length - 1 and bool((bases == 0x28).all())


def test_errors():
    codes = uniform_codes(9, 200, seed=5)
    lib = da.load()
    with da.Engine(0) as eng:
        h = eng._h
        with pytest.raises(da.DistanceError) as e:
            eng.pair_sites("raw", [0, 1], [1, 0])
        assert e.value.status == ERR_STATE
        eng.upload(0, codes)
        with pytest.raises(da.DistanceError) as e:
            eng.pair_sites("raw", [0, 3, 9, 12], [1, 2, 0, 0])
        assert e.value.status == ERR_ARG and "pair 2 " in e.value.message
        with pytest.raises(da.DistanceError) as e:
            eng.pair_sites("raw", [0, 3], [1, 9])
        assert e.value.status == ERR_ARG and "pair 1 " in e.value.message
        for s in (0, 1):
            with pytest.raises(da.DistanceError) as e:
                eng.pair_sites("raw", [0], [1], square=False, row_slot=s, col_slot=s)
            assert e.value.status == ERR_ARG
        with pytest.raises(da.DistanceError) as e:
            eng.pair_sites("raw", [0], [1], square=False, row_slot=0, col_slot=2)
        assert e.value.status == ERR_ARG
        with pytest.raises(da.DistanceError) as e:
            eng.pair_sites("raw", [0], [0], square=False, row_slot=0, col_slot=1)
        assert e.value.status == ERR_STATE
        row, col = np.array([0, 5, 2, 2], np.uint32), np.array([8, 1, 2, 7], np.uint32)
        want = expected("raw", codes, codes, row, col)
        total = int(want[0][-1])
        assert total > 2

        def call(measure=2, r=row, c=col, offsets=True, sites=True, bases=True, cap=total):
            off = np.full(row.size + 1, 77, np.uint64)
            s, b = np.zeros(total, np.uint32), np.zeros(total, np.uint8)
            tot = C.c_uint64(99)
            rc = lib.dst_pair_sites(h, measure, 1, 0, 1, None if r is None else r.ctypes.data, None if c is None else c.ctypes.data,
                                    row.size, off.ctypes.data if offsets else None, s.ctypes.data if sites else None,
                                    b.ctypes.data if bases else None, cap, C.byref(tot))
            return rc, off, s, b, int(tot.value)

        rc, off, s, b, tot = call()
        assert rc == 0 and tot == total
        assert_csr((off, s, b), want, "direct")
        rc, off, s, b, tot = call(cap=total - 1)
        assert rc == ERR_CAPACITY and tot == total and np.array_equal(off, want[0])
        rc, off, s, b, tot = call(sites=False, bases=False, cap=0)
        assert rc == 0 and tot == total and np.array_equal(off, want[0])
        assert call(sites=False)[0] == ERR_ARG and call(bases=False)[0] == ERR_ARG
        assert call(r=None)[0] == ERR_ARG and call(c=None)[0] == ERR_ARG and call(offsets=False)[0] == ERR_ARG
        assert call(measure=6)[0] == ERR_ARG and call(measure=-1)[0] == ERR_ARG
        eng.upload(1, uniform_codes(5, 90, seed=6))
        with pytest.raises(da.DistanceError) as e:
            eng.pair_sites("raw", [0], [0], square=False, row_slot=0, col_slot=1)
        assert e.value.status == ERR_STATE and "Different length sequences" in e.value.message
        assert_csr(eng.pair_sites("raw", row, col), want, "after the errors")
