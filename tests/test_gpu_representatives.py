"""GPU (-m gpu): dst_representatives / Engine.representatives, the greedy representatives of one set — rep, values (as
uint64 bits) and tallies exactly the sequential reference (representatives_reference.py) applied to the context's own
run_square values and tallies: every measure and kernel path, across row slabs and sub-blocks, on adversarial graphs (a
chain in input order, a permuted chain, a star, two hubs racing for the same members, ambiguity codes), with NaN values,
integer thresholds, tiny sets, every error status, and the consequences against Engine.clusters and Engine.links."""
import ctypes as C

import numpy as np
import pytest

import distance_amd as da
import representatives_reference as rr
from helpers import KNOWN, random_alignment, uniform_codes
from test_gpu_clusters import chain_codes, datasets, interior

pytestmark = pytest.mark.gpu
ALL = ("n", "n_high", "raw", "jc69", "k80", "tn93")
ERR_ARG, ERR_STATE, ERR_CAPACITY = 1, 4, 6
INF = float("inf")
BLOCK_ROWS = 512   # the sub-block height of dst_representatives.hip (kRepBlockRows)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def check(eng, m, t, vals, tal=None, max_pairs=0, note=None):
    """One call with values and tallies (the slab as DST_OUT_TALLY) and one with values alone (the slab as
    DST_OUT_DISTANCE) against the reference; returns rep."""
    n, _ = eng.set_info(0)
    want_rep, want_val, want_tal = rr.reference(m, vals, n, t, tal)
    rep, values = eng.representatives(m, t, max_pairs=max_pairs)
    assert rep.dtype == np.uint32 and rep.shape == (n,) and values.dtype == vals.dtype and values.shape == (n,)
    assert np.array_equal(rep, want_rep), (note, m, t, max_pairs)
    assert np.array_equal(bits(values), bits(want_val)), (note, m, t, max_pairs)
    assert eng.last_representatives == int((want_rep == np.arange(n)).sum())
    if tal is not None:
        rep2, values2, tallies = eng.representatives(m, t, max_pairs=max_pairs, tallies=True)
        assert tallies.dtype == np.uint32 and tallies.shape == want_tal.shape
        assert np.array_equal(rep2, want_rep), (note, m, t, max_pairs)
        assert np.array_equal(bits(values2), bits(want_val)), (note, m, t, max_pairs)
        assert np.array_equal(tallies, want_tal), (note, m, t, max_pairs)
    return rep


@pytest.fixture(scope="module")
def sets():
    return datasets()


# ---- 1. every measure on every path -------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["dense", "consensus", "hybrid"])
@pytest.mark.parametrize("kind", ["low", "clade", "nrun", "uniform"])
def test_every_measure_every_path(sets, path, kind):
    codes = sets[kind]
    with da.Engine(0) as eng:
        eng.set_prep_threshold(0)
        eng.set_path(path)
        eng.upload(0, codes)
        for m in ALL:
            vals = eng.run_square(m)
            tal = eng.run_square(m, tallies=True)
            for t in (0.0, interior(m, vals), INF):
                rep = check(eng, m, t, vals, tal, note=(path, kind))
            (alone,) = eng.representatives(m, t, values=False)   # rep alone: no values launch
            assert np.array_equal(alone, rep), (path, kind, m)


# ---- 2. the slab bound does not change the result ----------------------------------------------------------------------
def test_slab_sizes(sets):
    codes = sets["clade"]
    n = len(codes)
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        for m in ("n_high", "raw", "tn93"):
            vals = eng.run_square(m)
            tal = eng.run_square(m, tallies=True)
            t = interior(m, vals)
            for max_pairs in (1, n - 1, 3000, 0):   # one row per slab (1: the bound is below a row), a few rows, one slab
                check(eng, m, t, vals, tal, max_pairs=max_pairs)


# ---- 3. chains ------------------------------------------------------------------------------------------------------------
def test_chain_in_input_order():
    """The worst case of the serial part: every second record is a representative, each decided by the one before it."""
    n = 1500
    codes, perm = chain_codes(n, seed=71)
    ordered = np.ascontiguousarray(codes[perm])   # record k = position k of the chain
    want = (np.arange(n) // 2 * 2).astype(np.uint32)
    with da.Engine(0) as eng:
        eng.upload(0, ordered)
        vals = eng.run_square("n_high")
        tal = eng.run_square("n_high", tallies=True)
        for max_pairs in (1, 2000, 0):
            rep = check(eng, "n_high", 1, vals, tal, max_pairs=max_pairs)
            assert np.array_equal(rep, want), max_pairs
            _, values = eng.representatives("n_high", 1, max_pairs=max_pairs)
            assert np.array_equal(values, np.arange(n) % 2), max_pairs
        eng.upload(0, codes)   # the permuted chain
        vals = eng.run_square("n_high")
        tal = eng.run_square("n_high", tallies=True)
        for max_pairs in (1, 2000, 0):
            check(eng, "n_high", 1, vals, tal, max_pairs=max_pairs)


# ---- 4. the star ----------------------------------------------------------------------------------------------------------
def test_star():
    n, centre = 1200, 777
    rng = np.random.default_rng(72)
    root = rng.choice(np.array(KNOWN, np.uint8), size=n)
    codes = np.tile(root, (n, 1))
    leaf = 0
    for r in range(n):   # every leaf one site from the centre, a site of its own: two leaves are two sites apart
        if r != centre:
            codes[r, leaf] = KNOWN[(KNOWN.index(int(root[leaf])) + 1) % 4]
            leaf += 1
    own = np.arange(n, dtype=np.uint32)
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        vals = eng.run_square("n_high")
        for max_pairs in (1, 5000, 0):
            rep = check(eng, "n_high", 1, vals, max_pairs=max_pairs)
            want = own.copy()
            want[centre] = 0
            assert np.array_equal(rep, want), max_pairs
            rep = check(eng, "n_high", 2, vals, max_pairs=max_pairs)
            assert not rep.any(), max_pairs
            rep = check(eng, "n_high", 0.5, vals, max_pairs=max_pairs)
            assert np.array_equal(rep, own), max_pairs


# ---- 5. two hubs: the values race -------------------------------------------------------------------------------------------
def test_two_hubs():
    """a = record 0 and b = record 1 are three sites apart and both within 2 of every later record: rep is a's, and so are
    the value and the tallies, although b's row meets the same records in the same cover launch."""
    n, L = 700, 64
    rng = np.random.default_rng(76)
    root = rng.choice(np.array(KNOWN, np.uint8), size=L)
    other = np.array([KNOWN[(KNOWN.index(int(c)) + 1) % 4] for c in root], np.uint8)
    codes = np.tile(root, (n, 1))
    codes[1, :3] = other[:3]
    near_b = rng.random(n) < 0.5
    near_b[:2] = False
    codes[2:, 0] = other[0]
    codes[near_b, 1] = other[1]   # root + {0, 1}: 2 from a, 1 from b; the rest root + {0}: 1 from a, 2 from b
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        vals = eng.run_square("n_high")
        tal = eng.run_square("n_high", tallies=True)
        assert vals[0] == 3
        for max_pairs in (0, 1):   # a and b in one sub-block; in different slabs
            rep = check(eng, "n_high", 2, vals, tal, max_pairs=max_pairs)
            assert rep[0] == 0 and rep[1] == 1 and not rep[2:].any()
            _, values = eng.representatives("n_high", 2, max_pairs=max_pairs)
            assert np.array_equal(values[2:], np.where(near_b[2:], 2, 1)), max_pairs


# ---- 6. ambiguity: distance 0 is not transitive ----------------------------------------------------------------------------
def test_ambiguity():
    A, G, R = 136, 72, 192
    codes = np.full((3, 30), A, np.uint8)
    codes[1, 7], codes[2, 7] = R, G
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        vals = eng.run_square("n_high")
        assert list(vals) == [0, 1, 0]
        rep = check(eng, "n_high", 0, vals, eng.run_square("n_high", tallies=True))
        assert list(rep) == [0, 0, 2]
        labels, _ = eng.clusters("n_high", 0)
        assert list(labels) == [0, 0, 0]


# ---- 7. NaN never links ---------------------------------------------------------------------------------------------------
def test_nan_never_links():
    codes = uniform_codes(150, 40, seed=73)   # high divergence: jc69 / k80 / tn93 are NaN for many pairs
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        for m in ("jc69", "k80", "tn93"):
            vals = eng.run_square(m)
            tal = eng.run_square(m, tallies=True)
            assert np.isnan(vals).any(), m
            rep = check(eng, m, INF, vals, tal)
            assert (rep == np.arange(150)).sum() > 1, m   # (with +inf only NaN keeps a second representative)
            rep0 = check(eng, m, 0.0, vals, tal)
            rep_neg = check(eng, m, -0.0, vals, tal)      # -0.0 links wherever +0.0 does
            assert np.array_equal(rep0, rep_neg), m


# ---- 8. integer thresholds ---------------------------------------------------------------------------------------------
def test_integer_thresholds(sets):
    codes = sets["low"]
    n = len(codes)
    own = np.arange(n, dtype=np.uint32)
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        for m in ("n", "n_high"):
            vals = eng.run_square(m)
            t = float(np.quantile(vals, 0.05))
            a = check(eng, m, t, vals)
            b = check(eng, m, t + 0.75, vals)
            assert np.array_equal(a, b), m
            for neg in (-0.5, -1.0, -1e300, -INF):   # floor(T) < 0: nothing links (every count is >= 0)
                rep, values, tallies = eng.representatives(m, neg, tallies=True)
                assert np.array_equal(rep, own) and not values.any() and not tallies.any(), (m, neg)
                assert eng.last_representatives == n
            rep = check(eng, m, 1e300, vals)   # clamped to the int64 range: everything links
            assert not rep.any() and eng.last_representatives == 1


# ---- 9. several sub-blocks inside a slab and several default slabs ------------------------------------------------------------
def test_sub_blocks_and_slabs():
    """9,000 records: 40.5 M pairs, more than the 2^25 of a default slab, whose first slab holds more than 3,700 rows: seven
    sub-blocks of 512 rows and more in every slab."""
    n, L = 9000, 200
    assert n * (n - 1) // 2 > 1 << 25 and (1 << 25) // n >= 3 * BLOCK_ROWS
    rng = np.random.default_rng(79)
    root = rng.choice(np.array(KNOWN, np.uint8), size=L)
    codes = np.tile(root, (n, 1))
    for r in range(n):   # low diversity: zero to three changed sites per record
        sites = rng.choice(L, rng.integers(0, 4), replace=False)
        codes[r, sites] = rng.choice(np.array(KNOWN, np.uint8), len(sites))
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        vals = eng.run_square("n_high")
        rep = check(eng, "n_high", 1, vals, eng.run_square("n_high", tallies=True))
        kept = int((rep == np.arange(n)).sum())
        assert 1 < kept < n
        vals = eng.run_square("raw")
        check(eng, "raw", float(np.quantile(vals[::97], 0.01)), vals, eng.run_square("raw", tallies=True))


# ---- 10. tiny sets, errors, state left behind ---------------------------------------------------------------------------
def test_tiny_sets():
    codes = random_alignment(3, 50, seed=74)
    with da.Engine(0) as eng:
        eng.upload(0, codes[:1])
        rep, values, tallies = eng.representatives("raw", INF, tallies=True)
        assert list(rep) == [0] and bits(values)[0] == 0 and not tallies.any() and eng.last_representatives == 1
        eng.upload(0, np.ascontiguousarray(codes[[0, 0]]))
        vals = eng.run_square("raw")
        rep = check(eng, "raw", 0.0, vals, eng.run_square("raw", tallies=True))
        assert list(rep) == [0, 0] and eng.last_representatives == 1
        eng.upload(0, codes[:2])
        vals = eng.run_square("n_high")
        assert vals[0] > 0
        assert list(check(eng, "n_high", 0, vals, eng.run_square("n_high", tallies=True))) == [0, 1]
        assert list(check(eng, "n_high", -1, vals)) == [0, 1]
        assert list(check(eng, "n_high", INF, vals, eng.run_square("n_high", tallies=True))) == [0, 0]


def test_errors():
    lib = da.load()
    codes = random_alignment(50, 100, seed=75)
    rep = np.zeros(50, np.uint32)
    val = np.zeros(50, np.float64)
    tal = np.zeros((50, 2), np.uint32)
    nr = C.c_uint64(7)
    own = np.arange(50, dtype=np.uint32)

    def call(h, m, t, rep_p, cap, count=None, tal_p=None, val_p=None):
        return lib.dst_representatives(h, m, t, 0, rep_p, tal_p, val_p, cap, count)

    assert call(None, 2, 1.0, rep.ctypes.data, 50) == ERR_ARG
    with da.Engine(0) as eng:
        h = eng._h
        assert call(h, 2, 1.0, rep.ctypes.data, 50, C.byref(nr)) == ERR_STATE
        assert lib.dst_last_error(h) == b"set not uploaded" and nr.value == 0
        eng.upload(0, codes)
        assert call(h, 2, float("nan"), rep.ctypes.data, 50, C.byref(nr)) == ERR_ARG
        assert lib.dst_last_error(h) == b"threshold is NaN"
        assert call(h, 9, 1.0, rep.ctypes.data, 50, C.byref(nr)) == ERR_ARG
        assert lib.dst_last_error(h) == b"unknown measure"
        assert call(h, -1, 1.0, rep.ctypes.data, 50, C.byref(nr)) == ERR_ARG
        assert call(h, 2, 1.0, None, 50, C.byref(nr)) == ERR_ARG
        assert call(h, 2, 1.0, rep.ctypes.data, 49, C.byref(nr)) == ERR_CAPACITY
        assert lib.dst_last_error(h) == b"cap is below the set's record count"
        assert call(h, 2, 1.0, rep.ctypes.data, 49, C.byref(nr), tal.ctypes.data, val.ctypes.data) == ERR_CAPACITY
        assert call(h, 2, INF, rep.ctypes.data, 50, C.byref(nr), tal.ctypes.data, val.ctypes.data) == 0
        assert nr.value == 1 and not rep.any()
        vals = eng.run_square("raw")
        assert np.array_equal(bits(val)[1:], bits(vals[:49])) and bits(val)[0] == 0
        assert np.array_equal(tal[1:], eng.run_square("raw", tallies=True)[:49]) and not tal[0].any()
        assert call(h, 2, -1.0, rep.ctypes.data, 50) == 0   # every optional pointer NULL
        assert np.array_equal(rep, own)
        assert call(h, 2, -1.0, rep.ctypes.data, 50, C.byref(nr), tal.ctypes.data, val.ctypes.data) == 0
        assert nr.value == 50 and not bits(val).any() and not tal.any()


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
            eng.representatives(m, interior(m, before), max_pairs=2000, tallies=True)
            eng.representatives(m, interior(m, before), max_pairs=2000)
            after = eng.run_square(m)
            assert eng.last_path() == used
            assert np.array_equal(bits(before), bits(after)), (path, m)


# ---- 11. the consequences against Engine.clusters and Engine.links ---------------------------------------------------------------
def test_consequences_against_clusters_and_links(sets):
    for kind in ("low", "clade", "nrun", "uniform"):
        codes = sets[kind]
        n = len(codes)
        own = np.arange(n)
        with da.Engine(0) as eng:
            eng.upload(0, codes)
            for m in ("n_high", "raw", "tn93"):
                t = interior(m, eng.run_square(m))
                rep, _ = eng.representatives(m, t)
                labels, _ = eng.clusters(m, t)
                row, col = eng.links(m, t, values=False)
                is_rep = rep == own
                assert is_rep[0]
                assert not (is_rep[row] & is_rep[col]).any(), (kind, m)          # no link between two representatives
                assert is_rep[np.unique(labels)].all(), (kind, m)                # each cluster's smallest record is one
                assert np.array_equal(labels[rep], labels), (kind, m)            # a member lies in its representative's cluster
                assert is_rep.sum() >= len(np.unique(labels))
                # every member is linked to its representative, and to no smaller one
                first = np.full(n, n, np.int64)
                np.minimum.at(first, col[is_rep[row]], row[is_rep[row]])
                np.minimum.at(first, row[is_rep[col]], col[is_rep[col]])
                assert np.array_equal(first[~is_rep], rep[~is_rep]), (kind, m)
