"""GPU (-m gpu): neighbour-joining trees (dst_nj, dst_nj_matrix) against the numpy restatement of the contract
(nj_reference.py) bit for bit, on every measure and path, against generating trees of additive matrices, on the error
cases and at scale."""
import ctypes as C

import numpy as np
import pytest

import distance_amd as da
import nj_reference as R
from helpers import CODES, random_alignment
from tools import synth

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE, ERR_CAPACITY = 1, 4, 6


@pytest.fixture(scope="module")
def eng():
    with da.Engine(0) as e:
        yield e


def same_tree(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64))   # bits: -0.0 and NaN patterns included


def with_duplicates(n, L, seed):
    codes = random_alignment(n, L, seed=seed, divergence=0.03)
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n, n // 5)
    dst = rng.integers(0, n, n // 5)
    codes[dst] = codes[src]
    return np.ascontiguousarray(codes)


# ---- 1. bit-exact agreement with the restatement -------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 4, 5, 63, 64, 65, 255, 256, 257, 1500])
def test_random_matrices(eng, n):
    rng = np.random.default_rng(n)
    d = rng.random((n, n))
    d[np.tril_indices(n)] = rng.random(n * (n + 1) // 2) * 7   # never read
    got = eng.nj_matrix(d)
    R.check_tree(*got, n)
    same_tree(got, R.nj(d))


@pytest.mark.parametrize("kind", ["equal", "small_int", "duplicate_rows", "zeros", "negative_zero"])
def test_ties(eng, kind):
    n = 70
    rng = np.random.default_rng(5)
    if kind == "equal":
        d = np.full((n, n), 0.25)
    elif kind == "small_int":
        d = rng.integers(0, 4, (n, n)).astype(np.float64)
    elif kind == "duplicate_rows":
        base = rng.random((n // 4, n // 4))
        base = base + base.T
        pick = rng.integers(0, n // 4, n)
        d = base[np.ix_(pick, pick)]
    elif kind == "zeros":
        d = np.zeros((n, n))
    else:
        d = np.where(rng.random((n, n)) < 0.5, -0.0, 0.0)
    got = eng.nj_matrix(d)
    R.check_tree(*got, n)
    same_tree(got, R.nj(d))


def test_non_metric_negative_lengths(eng):
    n = 40
    rng = np.random.default_rng(11)
    d = rng.random((n, n)) * 100
    d[0, 1:] = 1e-3            # far closer than any triangle inequality allows
    d[1:5, 5:] = 500.0
    got = eng.nj_matrix(d)
    assert (got[1] < 0).any()
    same_tree(got, R.nj(d))


@pytest.mark.parametrize("n", [17, 100, 700])
def test_compactions(eng, n):
    """sizes whose rounds cross several compactions (m <= floor(3P/4)), integer values: exact in f64"""
    d = np.random.default_rng(n).integers(0, 50, (n, n)).astype(np.float64)
    same_tree(eng.nj_matrix(d), R.nj(d))


# ---- 2. every measure, every path --------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", ["n", "n_high", "raw", "jc69", "k80", "tn93"])
def test_measures(eng, measure):
    codes = with_duplicates(150, 600, seed=21)
    eng.upload(0, codes)
    got = eng.nj(measure)
    D = R.square(150, eng.run_square(measure))
    same_tree(got, eng.nj_matrix(D))
    same_tree(got, R.nj(D))


@pytest.mark.parametrize("measure", ["n", "raw", "tn93"])
def test_path_independence(eng, measure):
    codes = with_duplicates(300, 500, seed=22)
    eng.upload(0, codes)
    try:
        eng.set_path("auto")
        want = eng.nj(measure)
        for path in ("dense", "consensus"):
            eng.set_path(path)
            same_tree(eng.nj(measure), want)
        eng.set_path("auto")
        for max_pairs in (1, 299, 5000):   # one row per slab; many slabs: the mirror across slabs
            same_tree(eng.nj(measure, max_pairs=max_pairs), want)
    finally:
        eng.set_path("auto")


# ---- 3. additive trees: the generating tree, independently of the restatement --------------------------------------
@pytest.mark.parametrize("shape,n", [("random", 5), ("random", 300), ("random", 2000), ("caterpillar", 500),
                                     ("caterpillar", 3000), ("balanced", 1024), ("random", 8192)])
def test_additive_recovery(eng, shape, n):
    rng = np.random.default_rng(n + len(shape))
    parent, length = R.random_tree(n, shape, rng)
    D = R.path_matrix(parent, length, n)
    got = eng.nj_matrix(D)
    R.check_tree(*got, n)
    assert R.splits(*got, n) == R.splits(parent, length, n)


# ---- 4. errors ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_matrix_non_finite(eng, bad):
    d = np.ones((10, 10))
    d[3, 7] = bad
    with pytest.raises(da.DistanceError) as e:
        eng.nj_matrix(d)
    assert e.value.status == ERR_ARG and "3 and 7" in e.value.message
    d[3, 7] = 1.0
    d[7, 3] = bad             # the lower triangle is never read
    R.check_tree(*eng.nj_matrix(d), 10)


def test_set_non_finite(eng):
    codes = random_alignment(20, 50, seed=3)
    codes[4] = CODES[14]      # all N: raw has no comparable site with any record, NaN
    eng.upload(0, codes)
    with pytest.raises(da.DistanceError) as e:
        eng.nj("raw")
    assert e.value.status == ERR_STATE and "records 0 and 4" in e.value.message
    R.check_tree(*eng.nj("n"), 20)   # integer measures are finite


def test_small_and_args(eng):
    lib, h = da.load(), eng._h
    p, ln = np.zeros(8, np.uint32), np.zeros(8)
    for n in (0, 1, 2):
        assert lib.dst_nj_matrix(h, np.zeros(max(n * n, 1)).ctypes.data, n, p.ctypes.data, ln.ctypes.data, 8) == ERR_ARG
    d = np.ones((5, 5))
    assert lib.dst_nj_matrix(h, d.ctypes.data, 5, p.ctypes.data, ln.ctypes.data, 7) == ERR_CAPACITY
    assert lib.dst_nj_matrix(h, d.ctypes.data, 5, None, ln.ctypes.data, 8) == ERR_ARG
    assert lib.dst_nj_matrix(h, d.ctypes.data, 5, p.ctypes.data, None, 8) == ERR_ARG
    assert lib.dst_nj_matrix(h, None, 5, p.ctypes.data, ln.ctypes.data, 8) == ERR_ARG
    assert lib.dst_nj_matrix(h, d.ctypes.data, 5, p.ctypes.data, ln.ctypes.data, 8) == 0
    eng.upload(0, random_alignment(2, 30, seed=1))
    assert lib.dst_nj(h, 2, 0, p.ctypes.data, ln.ctypes.data, 8) == ERR_ARG
    eng.upload(0, random_alignment(5, 30, seed=1))
    assert lib.dst_nj(h, 2, 0, p.ctypes.data, ln.ctypes.data, 7) == ERR_CAPACITY
    assert lib.dst_nj(h, 9, 0, p.ctypes.data, ln.ctypes.data, 8) == ERR_ARG
    assert lib.dst_nj(h, 2, 0, None, ln.ctypes.data, 8) == ERR_ARG
    assert lib.dst_nj(h, 2, 0, p.ctypes.data, ln.ctypes.data, 8) == 0
    with da.Engine(0) as fresh:
        assert lib.dst_nj(fresh._h, 2, 0, p.ctypes.data, ln.ctypes.data, 8) == ERR_STATE


# ---- 5. scale ----------------------------------------------------------------------------------------------------
def test_scale_20000(eng):
    n = 20000
    eng.upload(0, synth.alignment(synth.SEED ^ 11, n, 30000))
    a = eng.nj("raw")
    R.check_tree(*a, n)
    same_tree(eng.nj("raw"), a)
