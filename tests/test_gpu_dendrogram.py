"""GPU (-m gpu): dendrograms (dst_dendrogram, dst_dendrogram_matrix) against the numpy restatement of the contract
(dendrogram_reference.py) bit for bit — parent, length and height, for UPGMA, WPGMA and complete linkage — on random
matrices at workgroup edges, on ties, on matrices built to invalidate the row-minimum cache, through the tail, from
alignments on every measure and path, against the max / mean properties of the input, on the error cases and at scale."""
import time

import numpy as np
import pytest

import distance_amd as da
import dendrogram_reference as R
from helpers import CODES, random_alignment
from tools import synth

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE, ERR_CAPACITY = 1, 4, 6
LINKAGES = R.LINKAGES


@pytest.fixture(scope="module")
def eng():
    with da.Engine(0) as e:
        yield e


def same_tree(got, want):
    assert np.array_equal(got[0], want[0])
    for g, w in zip(got[1:3], want[1:3]):
        assert np.array_equal(g.view(np.uint64), w.view(np.uint64))   # bits: -0.0 included


def check(eng, d, linkage):
    """one matrix, one linkage: the GPU's tree is the restatement's; returns row_scans"""
    n = d.shape[0]
    got = eng.dendrogram_matrix(d, linkage, stats=True)
    R.check_tree(*got[:3], n)
    same_tree(got, R.dendrogram(d, linkage))
    return got[3]


def with_duplicates(n, L, seed, codes=None):
    codes = random_alignment(n, L, seed=seed, divergence=0.03) if codes is None else codes.copy()
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n, n // 5)
    dst = rng.integers(0, n, n // 5)
    codes[dst] = codes[src]
    return np.ascontiguousarray(codes)


# ---- 1. bit-exact agreement with the restatement -------------------------------------------------------------------
@pytest.mark.parametrize("linkage", LINKAGES)
@pytest.mark.parametrize("n", [2, 3, 4, 63, 64, 65, 255, 256, 257, 1500])
def test_random_matrices(eng, n, linkage):
    rng = np.random.default_rng(n)
    d = rng.random((n, n))
    d[np.tril_indices(n)] = rng.random(n * (n + 1) // 2) * 7   # never read
    check(eng, d, linkage)


@pytest.mark.parametrize("linkage", LINKAGES)
@pytest.mark.parametrize("kind", ["equal", "small_int", "duplicate_rows", "zeros", "negative_zero"])
def test_ties(eng, kind, linkage):
    n = 300
    rng = np.random.default_rng(5)
    if kind == "equal":
        d = np.full((n, n), 0.25)
    elif kind == "small_int":
        d = rng.integers(0, 4, (n, n)).astype(np.float64)
    elif kind == "duplicate_rows":
        base = rng.random((n // 4, n // 4))
        base = base + base.T
        np.fill_diagonal(base, 0.0)
        pick = rng.integers(0, n // 4, n)
        d = base[np.ix_(pick, pick)]
    elif kind == "zeros":
        d = np.zeros((n, n))
    else:
        d = np.where(rng.random((n, n)) < 0.5, -0.0, 0.0)
    check(eng, d, linkage)


def invalidation_matrix(kind, n):
    rng = np.random.default_rng(17)
    if kind in ("hub_last", "hub_first"):
        # every record's nearest record is the hub: every row's cached column (hub last), or every row's one changed
        # entry (hub first), goes with the first merge
        d = 10.0 + rng.random((n, n))
        d = np.triu(d, 1) + np.triu(d, 1).T
        hub = n - 1 if kind == "hub_last" else 0
        near = 1.0 + rng.random(n)
        d[hub, :] = near
        d[:, hub] = near
        return d
    if kind == "chain":
        pos = rng.permutation(n).astype(np.float64)
        return np.abs(pos[:, None] - pos[None, :])
    # two tight clades far apart, interleaved in record order
    side = rng.integers(0, 2, n)
    d = rng.random((n, n)) * 0.01
    d = np.triu(d, 1) + np.triu(d, 1).T
    return d + 100.0 * (side[:, None] != side[None, :])


@pytest.mark.parametrize("linkage", LINKAGES)
@pytest.mark.parametrize("kind", ["hub_last", "hub_first", "chain", "two_clades"])
def test_cache_invalidation(eng, kind, linkage):
    n = 500
    scans = check(eng, invalidation_matrix(kind, n), linkage)
    print(f"row_scans {kind} {linkage} n={n}: {scans} ({scans / (n - 1):.2f} per round)")
    assert scans >= n - 1


@pytest.mark.parametrize("linkage", LINKAGES)
def test_tail(eng, linkage):
    """n = 700: the last rounds run over rows that are mostly dead slots, skipped by the active flag; every round is
    compared (the whole tree is)"""
    d = np.random.default_rng(700).integers(0, 50, (700, 700)).astype(np.float64)
    scans = check(eng, d, linkage)
    print(f"row_scans tail {linkage} n=700: {scans}")


# ---- 2. from alignments: every measure, every path, every slab cut ---------------------------------------------------
@pytest.mark.parametrize("source", ["random", "synth"])
@pytest.mark.parametrize("measure", ["n", "n_high", "raw", "jc69", "k80", "tn93"])
def test_measures(eng, measure, source):
    n, L = 300, 400
    codes = with_duplicates(n, L, 21, None if source == "random" else synth.alignment(synth.SEED ^ 5, n, L))
    eng.upload(0, codes)
    D = R.square(n, eng.run_square(measure))
    for linkage in LINKAGES:
        got = eng.dendrogram(measure, linkage)
        same_tree(got, eng.dendrogram_matrix(D, linkage))
        same_tree(got, R.dendrogram(D, linkage))


@pytest.mark.parametrize("measure", ["n", "raw", "tn93"])
def test_path_and_slab_independence(eng, measure):
    codes = with_duplicates(300, 400, seed=22)
    eng.upload(0, codes)
    try:
        for linkage in LINKAGES:
            eng.set_path("auto")
            want = eng.dendrogram(measure, linkage)
            for path in ("dense", "consensus"):
                eng.set_path(path)
                same_tree(eng.dendrogram(measure, linkage), want)
            eng.set_path("auto")
            for max_pairs in (0, 1000, 37):
                same_tree(eng.dendrogram(measure, linkage, max_pairs=max_pairs), want)
    finally:
        eng.set_path("auto")


# ---- 3. properties of the input, independently of the restatement ---------------------------------------------------
def node_sizes(parent, n):
    size = np.ones(2 * n - 1, np.int64)
    size[n:] = 0
    for x in range(2 * n - 2):
        size[parent[x]] += size[x]
    return size


def test_linkage_properties_4000(eng):
    n = 4000
    eng.upload(0, with_duplicates(n, 2000, seed=23))
    D = R.square(n, eng.run_square("n"))
    parent, length, height = eng.dendrogram("n", "complete")
    R.check_tree(parent, length, height, n)
    below, kids = R.leaf_sets(parent, n)
    for u in range(n, 2 * n - 1):
        cross = D[np.ix_(below[kids[u][0]], below[kids[u][1]])]
        assert (height[u] * 2.0).view(np.uint64) == cross.max().view(np.uint64), u
    assert (np.diff(height[n:]) >= 0).all()
    parent, length, height = eng.dendrogram("n", "average")
    R.check_tree(parent, length, height, n)
    below, kids = R.leaf_sets(parent, n)
    for u in range(n, 2 * n - 1):
        mean = D[np.ix_(below[kids[u][0]], below[kids[u][1]])].mean()
        assert abs(height[u] * 2.0 - mean) <= 1e-12 * mean, u


def test_structure_20000(eng):
    n = 20000
    eng.upload(0, synth.alignment(synth.SEED ^ 11, n, 1000))
    for linkage in ("complete", "average"):
        t0 = time.perf_counter()
        parent, length, height, scans = eng.dendrogram("raw", linkage, stats=True)
        ms = (time.perf_counter() - t0) * 1e3
        print(f"dendrogram 20,000 x 1,000 raw {linkage}: {ms:.1f} ms, row_scans {scans}")
        R.check_tree(parent, length, height, n)
        size = node_sizes(parent, n)
        assert size[2 * n - 2] == n and (size[n:] >= 2).all()
        if linkage == "complete":
            assert (np.diff(height[n:]) >= 0).all()


# ---- 4. errors ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_matrix_non_finite(eng, bad):
    d = np.ones((10, 10))
    d[3, 7] = bad
    with pytest.raises(da.DistanceError) as e:
        eng.dendrogram_matrix(d)
    assert e.value.status == ERR_ARG and "3 and 7" in e.value.message
    d[3, 7] = 1.0
    d[7, 3] = bad             # the lower triangle is never read
    R.check_tree(*eng.dendrogram_matrix(d), 10)


def test_set_non_finite(eng):
    codes = random_alignment(20, 50, seed=3)
    codes[4] = CODES[14]      # all N: raw has no comparable site with any record, NaN
    eng.upload(0, codes)
    with pytest.raises(da.DistanceError) as e:
        eng.dendrogram("raw", "complete")
    assert e.value.status == ERR_STATE and "records 0 and 4" in e.value.message
    R.check_tree(*eng.dendrogram("n"), 20)   # integer measures are finite


def test_small_and_args(eng):
    lib, h = da.load(), eng._h
    p, ln, hg = np.zeros(9, np.uint32), np.zeros(9), np.zeros(9)
    P, L, H = p.ctypes.data, ln.ctypes.data, hg.ctypes.data
    for n in (0, 1):
        assert lib.dst_dendrogram_matrix(h, np.zeros(1).ctypes.data, n, 0, P, L, H, 9, None) == ERR_ARG
    d = np.ones((5, 5))
    for linkage in (-1, 3, 99):
        assert lib.dst_dendrogram_matrix(h, d.ctypes.data, 5, linkage, P, L, H, 9, None) == ERR_ARG
    assert lib.dst_dendrogram_matrix(h, d.ctypes.data, 5, 0, P, L, H, 8, None) == ERR_CAPACITY
    assert lib.dst_dendrogram_matrix(h, d.ctypes.data, 5, 0, None, L, H, 9, None) == ERR_ARG
    assert lib.dst_dendrogram_matrix(h, d.ctypes.data, 5, 0, P, None, H, 9, None) == ERR_ARG
    assert lib.dst_dendrogram_matrix(h, None, 5, 0, P, L, H, 9, None) == ERR_ARG
    assert lib.dst_dendrogram_matrix(h, d.ctypes.data, 5, 0, P, L, None, 9, None) == 0      # height may be NULL
    assert lib.dst_dendrogram_matrix(h, d.ctypes.data, 5, 2, P, L, H, 9, None) == 0
    with pytest.raises(ValueError):
        eng.dendrogram_matrix(d, "single")
    eng.upload(0, random_alignment(1, 30, seed=1))
    assert lib.dst_dendrogram(h, 2, 0, 0, P, L, H, 9, None) == ERR_ARG
    eng.upload(0, random_alignment(5, 30, seed=1))
    assert lib.dst_dendrogram(h, 2, 0, 0, P, L, H, 8, None) == ERR_CAPACITY
    assert lib.dst_dendrogram(h, 9, 0, 0, P, L, H, 9, None) == ERR_ARG
    assert lib.dst_dendrogram(h, 2, 3, 0, P, L, H, 9, None) == ERR_ARG
    assert lib.dst_dendrogram(h, 2, 0, 0, None, L, H, 9, None) == ERR_ARG
    assert lib.dst_dendrogram(h, 2, 0, 0, P, L, None, 9, None) == 0
    with da.Engine(0) as fresh:
        assert lib.dst_dendrogram(fresh._h, 2, 0, 0, P, L, H, 9, None) == ERR_STATE


# ---- 5. side effects -----------------------------------------------------------------------------------------------
def test_later_results_untouched(eng):
    codes = with_duplicates(200, 300, seed=31)
    eng.upload(0, codes)
    before = {m: eng.run_square(m) for m in ("n", "raw", "tn93")}
    a = eng.dendrogram("tn93", "average")
    eng.dendrogram_matrix(np.random.default_rng(1).random((50, 50)), "complete")
    for m, want in before.items():
        got = eng.run_square(m)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), m
    same_tree(eng.dendrogram("tn93", "average"), a)
    assert eng.set_info(0)[0] == 200
