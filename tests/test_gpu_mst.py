"""GPU (-m gpu): dst_mst / Engine.mst, the minimum spanning forest of one set — exactly Kruskal's forest
(tests/mst_reference.py) over the context's own run_square values: edges, values (bitwise) and tallies, on every measure
and kernel path, across row slabs, on adversarial graphs (a permuted chain, a star, identical records), with NaN values,
tiny sets, every error status, and its cut property against dst_clusters."""
import ctypes as C

import numpy as np
import pytest

import distance_amd as da
from helpers import KNOWN, random_alignment, uniform_codes
from mst_reference import components, kruskal, linked
from test_gpu_clusters import chain_codes, datasets, interior
from tools import synth

pytestmark = pytest.mark.gpu
ALL = ("n", "n_high", "raw", "jc69", "k80", "tn93")
ERR_ARG, ERR_STATE, ERR_CAPACITY = 1, 4, 6
INF = float("inf")
N_CODE = 240


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def canonical(n, edges):
    i, j = edges[:, 0].astype(np.int64), edges[:, 1].astype(np.int64)
    return i * (2 * n - i - 1) // 2 + (j - i - 1)


def check(eng, m, n, want, max_pairs=0, all_tallies=None, tag=None):
    """Engine.mst against the reference forest `want` = kruskal(n, run_square values); returns the rounds."""
    edges, values, rounds, tal = eng.mst(m, max_pairs=max_pairs, tallies=True)
    assert edges.dtype == np.uint32 and edges.shape == (len(want[0]), 2), (tag, m, edges.shape, want[0].shape)
    assert np.array_equal(edges.astype(np.int64), want[0]), (tag, m, max_pairs)
    assert values.dtype == want[1].dtype
    assert np.array_equal(bits(values), bits(want[1])), (tag, m, max_pairs)
    if all_tallies is not None:
        assert np.array_equal(tal, all_tallies[canonical(n, want[0])]), (tag, m, max_pairs)
    plain = eng.mst(m, max_pairs=max_pairs)
    assert len(plain) == 3 and np.array_equal(plain[0], edges) and np.array_equal(bits(plain[1]), bits(values))
    assert plain[2] == rounds
    assert rounds <= max(int(np.ceil(np.log2(max(n, 2)))), 1)
    return rounds


# ---- 1. every measure on every path -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sets():
    return datasets()


@pytest.fixture(scope="module")
def forests():
    """The reference forests, computed once per (dataset, measure): the values are bit-identical on every path."""
    return {}


def forest_of(forests, kind, m, n, vals):
    hit = forests.get((kind, m))
    if hit is None or not np.array_equal(bits(hit[0]), bits(vals)):
        hit = (vals.copy(), kruskal(n, vals))
        forests[(kind, m)] = hit
    return hit[1]


@pytest.mark.parametrize("path", ["dense", "consensus", "hybrid"])
@pytest.mark.parametrize("kind", ["low", "clade", "nrun", "uniform"])
def test_every_measure_every_path(sets, forests, path, kind):
    codes = sets[kind]
    n = len(codes)
    with da.Engine(0) as eng:
        eng.set_prep_threshold(0)
        eng.set_path(path)
        eng.upload(0, codes)
        for m in ALL:
            vals = eng.run_square(m)
            want = forest_of(forests, kind, m, n, vals)
            check(eng, m, n, want, all_tallies=eng.run_square(m, tallies=True), tag=(path, kind))


# ---- 2. the slab bound does not change the result ----------------------------------------------------------------------
def test_slab_sizes(sets, forests):
    codes = sets["clade"]
    n = len(codes)
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        for m in ("n_high", "raw", "tn93"):
            vals = eng.run_square(m)
            want = forest_of(forests, "clade", m, n, vals)
            tal = eng.run_square(m, tallies=True)
            for max_pairs in (1, n - 1, 3000, 0):   # one row per slab (1: the bound is below a row), a few thousand, default
                check(eng, m, n, want, max_pairs=max_pairs, all_tallies=tal, tag="slabs")


# ---- 3. adversarial graphs ---------------------------------------------------------------------------------------------
def test_permuted_chain():
    """All n - 1 edges have value 1: the order rests on (i, j) alone, and the components grow along the chain."""
    n = 1500
    codes, perm = chain_codes(n, seed=71)
    a, b = perm[:-1].astype(np.int64), perm[1:].astype(np.int64)
    chain = np.stack([np.minimum(a, b), np.maximum(a, b)], axis=1)
    chain = chain[np.lexsort((chain[:, 1], chain[:, 0]))]
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        vals = eng.run_square("n_high")
        want = kruskal(n, vals)
        assert np.array_equal(want[0], chain) and (want[1] == 1).all()
        for max_pairs in (2000, 0):
            rounds = check(eng, "n_high", n, want, max_pairs=max_pairs, tag="chain")
            assert rounds > 1
        rvals = eng.run_square("raw")
        rwant = kruskal(n, rvals)
        assert np.array_equal(rwant[0], chain)
        assert check(eng, "raw", n, rwant, tag="chain") > 1


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
    star = np.array([[min(r, centre), max(r, centre)] for r in range(n) if r != centre], np.int64)
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        want = kruskal(n, eng.run_square("n_high"))
        assert np.array_equal(want[0], star)
        for max_pairs in (5000, 0):
            check(eng, "n_high", n, want, max_pairs=max_pairs, tag="star")


def test_identical_records():
    n = 300
    codes = np.tile(random_alignment(1, 200, seed=76), (n, 1))
    star = np.stack([np.zeros(n - 1, np.int64), np.arange(1, n, dtype=np.int64)], axis=1)
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        for m in ("n_high", "raw", "jc69"):   # (jc69 of identical records is -0.0: the key of +0.0)
            want = kruskal(n, eng.run_square(m))
            assert np.array_equal(want[0], star)
            assert check(eng, m, n, want, tag="identical") == 1


# ---- 4. NaN is never an edge -------------------------------------------------------------------------------------------
def test_all_n_record_is_in_no_edge():
    n, dead = 90, 37
    codes = random_alignment(n, 300, seed=77)
    codes[dead, :] = N_CODE   # raw of a pair without a site where both are known: 0 / 0
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        vals = eng.run_square("raw")
        assert int(np.isnan(vals).sum()) == n - 1
        want = kruskal(n, vals)
        edges, values, _ = eng.mst("raw")
        assert len(edges) == n - 2 and dead not in edges
        check(eng, "raw", n, want, all_tallies=eng.run_square("raw", tallies=True), tag="all-N")


def test_nan_values():
    codes = uniform_codes(150, 40, seed=73)   # high divergence: jc69 / k80 / tn93 are NaN for many pairs
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        for m in ("jc69", "k80", "tn93"):
            vals = eng.run_square(m)
            assert np.isnan(vals).any(), m
            want = kruskal(150, vals)
            assert not np.isnan(want[1]).any()
            check(eng, m, 150, want, all_tallies=eng.run_square(m, tallies=True), tag="nan")
            assert len(want[0]) == 150 - len(np.unique(eng.clusters(m, INF)[0]))


# ---- 5. tiny sets, errors, state left behind ---------------------------------------------------------------------------
def test_tiny_sets():
    codes = random_alignment(3, 50, seed=74)
    with da.Engine(0) as eng:
        eng.upload(0, codes[:1])
        edges, values, rounds = eng.mst("raw")
        assert edges.shape == (0, 2) and len(values) == 0 and rounds == 0
        for k in (2, 3):
            eng.upload(0, codes[:k])
            for m in ALL:
                want = kruskal(k, eng.run_square(m))
                assert len(want[0]) == k - 1
                assert check(eng, m, k, want, all_tallies=eng.run_square(m, tallies=True), tag=k) >= 1


def test_errors():
    lib = da.load()
    codes = random_alignment(50, 100, seed=75)
    ei, ej = np.zeros(49, np.uint32), np.zeros(49, np.uint32)
    ne, nr = C.c_uint64(7), C.c_uint32(7)
    with da.Engine(0) as eng:
        h = eng._h
        p_i, p_j = ei.ctypes.data, ej.ctypes.data
        assert lib.dst_mst(h, 2, 0, p_i, p_j, None, None, 49, C.byref(ne), C.byref(nr)) == ERR_STATE
        assert ne.value == 0 and nr.value == 0
        eng.upload(0, codes)
        assert lib.dst_mst(h, 9, 0, p_i, p_j, None, None, 49, C.byref(ne), C.byref(nr)) == ERR_ARG
        assert lib.dst_mst(h, -1, 0, p_i, p_j, None, None, 49, C.byref(ne), C.byref(nr)) == ERR_ARG
        assert lib.dst_mst(h, 2, 0, None, p_j, None, None, 49, C.byref(ne), C.byref(nr)) == ERR_ARG
        assert lib.dst_mst(h, 2, 0, p_i, None, None, None, 49, C.byref(ne), C.byref(nr)) == ERR_ARG
        assert lib.dst_mst(h, 2, 0, p_i, p_j, None, None, 48, C.byref(ne), C.byref(nr)) == ERR_CAPACITY
        assert lib.dst_mst(h, 2, 0, p_i, p_j, None, None, 0, C.byref(ne), C.byref(nr)) == ERR_CAPACITY
        assert lib.dst_mst(h, 2, 0, p_i, p_j, None, None, 49, C.byref(ne), C.byref(nr)) == 0
        assert ne.value == 49 and nr.value >= 1
        want = kruskal(50, eng.run_square("raw"))
        assert np.array_equal(np.stack([ei, ej], axis=1).astype(np.int64), want[0])   # without values and tallies
        ei[:] = 0
        assert lib.dst_mst(h, 2, 0, p_i, p_j, None, None, 49, None, None) == 0
        assert np.array_equal(np.stack([ei, ej], axis=1).astype(np.int64), want[0])
        eng.upload(0, codes[:1])   # n < 2: ok whatever the room
        assert lib.dst_mst(h, 2, 0, p_i, p_j, None, None, 0, C.byref(ne), C.byref(nr)) == 0
        assert ne.value == 0 and nr.value == 0


@pytest.mark.parametrize("path", ["auto", "dense", "consensus"])
def test_run_square_unchanged(sets, path):
    codes = sets["nrun"]
    with da.Engine(0) as eng:
        eng.set_prep_threshold(0)
        eng.set_path(path)
        eng.upload(0, codes)
        for m in ("raw", "tn93"):
            before = eng.run_square(m)
            eng.mst(m, max_pairs=2000, tallies=True)
            after = eng.run_square(m)
            assert np.array_equal(bits(before), bits(after)), (path, m)


# ---- 6. the cut property: the forest's edges up to T span dst_clusters(T)'s clusters ---------------------------------------
def cut_labels(n, edges, values, t):
    keep = linked(values, t)
    return components(n, edges[keep, 0], edges[keep, 1])


def test_cut_property(sets):
    codes = sets["clade"]
    n = len(codes)
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        for m in ALL:
            edges, values, _ = eng.mst(m)
            for t in (0.0, interior(m, eng.run_square(m)), INF):
                assert np.array_equal(cut_labels(n, edges, values, t), eng.clusters(m, t)[0]), (m, t)


def test_mid_size_several_slabs():
    n, L = 5000, 2000
    codes = synth.alignment(synth.SEED ^ 11, n, L)
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        for m in ("n_high", "tn93"):
            edges, values, rounds = eng.mst(m, max_pairs=2 ** 21)   # 12.5 M pairs: six slabs a round
            assert (edges[:, 0] < edges[:, 1]).all()
            labels_inf = eng.clusters(m, INF)[0]
            assert len(edges) == n - len(np.unique(labels_inf))
            finite = values[np.isfinite(values)] if values.dtype == np.float64 else values
            for t in (0.0, float(np.quantile(finite, 0.3)), float(np.quantile(finite, 0.9)), INF):
                assert np.array_equal(cut_labels(n, edges, values, t), eng.clusters(m, t)[0]), (m, t)
            assert 1 <= rounds <= 13
