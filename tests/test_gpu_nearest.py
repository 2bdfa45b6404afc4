"""GPU (-m gpu): dst_nearest / Engine.nearest, the k nearest records of every record — exact against the oracle and
against the context's own full runs, on every kernel path, across several row slabs, with ties, and its errors."""
import ctypes as C

import numpy as np
import pytest

import distance_amd as da
import oracle
from helpers import random_alignment, uniform_codes
from tools import synth

pytestmark = pytest.mark.gpu
ALL = ("n", "n_high", "raw", "jc69", "k80", "tn93")
SLAB_PAIRS = 1 << 25   # the slab bound dst_nearest documents (kNearestSlabPairs)
ERR_ARG, ERR_STATE, ERR_CAPACITY = 1, 4, 6


def keys(vals: np.ndarray) -> np.ndarray:
    """The documented sort key of DST_OUT_DISTANCE payloads."""
    vals = np.ascontiguousarray(vals)
    if vals.dtype == np.int64:
        return vals.view(np.uint64) ^ np.uint64(1 << 63)
    b = vals.view(np.uint64)
    k = np.where((b >> np.uint64(63)) == 1, ~b, b | np.uint64(1 << 63))
    k[vals == 0] = np.uint64(1 << 63)
    k[np.isnan(vals)] = np.uint64(0xFFFFFFFFFFFFFFFF)
    return k


def smallest(key_row: np.ndarray, k: int, exclude: int = -1) -> np.ndarray:
    """Indices of the k smallest (key, index) of one row, in that order (`exclude`: a column left out)."""
    idx = np.arange(len(key_row))
    if exclude >= 0:
        idx = np.delete(idx, exclude)
    kr = key_row[idx]
    k = min(k, len(idx))
    if k == 0:
        return idx[:0]
    kth = np.partition(kr, k - 1)[k - 1]
    cand = np.nonzero(kr <= kth)[0]
    order = cand[np.lexsort((idx[cand], kr[cand]))][:k]
    return idx[order]


def square_matrix(cond: np.ndarray, n: int) -> np.ndarray:
    """Full n x n matrix (diagonal 0) of a condensed canonical-order square result."""
    m = np.zeros((n, n) + cond.shape[1:], cond.dtype)
    iu = np.triu_indices(n, 1)
    m[iu] = cond
    m[(iu[1], iu[0])] = cond
    return m


def canon(n: int, i: np.ndarray, j: np.ndarray) -> np.ndarray:
    a, b = np.minimum(i, j).astype(np.int64), np.maximum(i, j).astype(np.int64)
    return a * (2 * n - a - 1) // 2 + b - a - 1


def as_payload(measure, vals):
    return vals.astype(np.int64) if measure in da.INT_MEASURES else vals


def expected_square(vals_cond, n, k):
    full = keys(square_matrix(vals_cond, n))
    return np.array([smallest(full[i], k, exclude=i) for i in range(n)]).reshape(n, -1)


# ---- 1. exact against the oracle --------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", ["n", "n_high", "raw"])
def test_square_exact_against_oracle(measure):
    codes = random_alignment(300, 500, seed=11)
    want = as_payload(measure, oracle.all_pairs_square(measure, codes))
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        for k in (1, 5, 256):
            idx, vals = eng.nearest(measure, k)
            assert idx.shape == (300, k)
            exp = expected_square(want, 300, k)
            assert np.array_equal(idx, exp), (measure, k)
            rows = np.repeat(np.arange(300), k).reshape(300, k)
            assert np.array_equal(vals.view(np.uint64), want[canon(300, rows, idx)].view(np.uint64)), (measure, k)
        for k in (299, 1000):   # beyond the documented 1 <= k <= 256
            with pytest.raises(da.DistanceError) as e:
                eng.nearest(measure, k)
            assert e.value.status == ERR_ARG
    # fewer candidates than k: k_used = n - 1
    small = random_alignment(40, 300, seed=12)
    want = as_payload(measure, oracle.all_pairs_square(measure, small))
    with da.Engine(0) as eng:
        eng.upload(0, small)
        idx, vals = eng.nearest(measure, 100)
        assert idx.shape == (40, 39)
        assert np.array_equal(idx, expected_square(want, 40, 39))


@pytest.mark.parametrize("measure", ["n", "n_high", "raw"])
def test_rect_exact_against_oracle(measure):
    a = random_alignment(200, 400, seed=21)
    b = random_alignment(700, 400, seed=22)
    want = as_payload(measure, oracle.all_pairs_rect(measure, a, b))
    kk = keys(want)
    with da.Engine(0) as eng:
        eng.upload(0, a)
        eng.upload(1, b)
        for k in (1, 5, 256):
            idx, vals = eng.nearest(measure, k, square=False, row_slot=0, col_slot=1)
            exp = np.array([smallest(kk[i], k) for i in range(200)])
            assert np.array_equal(idx, exp), (measure, k)
            assert np.array_equal(vals.view(np.uint64), np.take_along_axis(want, idx.astype(np.int64), 1).view(np.uint64))
        # the other way round: rows of slot 1
        idx, _ = eng.nearest(measure, 3, square=False, row_slot=1, col_slot=0)
        kt = keys(np.ascontiguousarray(want.T))
        assert np.array_equal(idx, np.array([smallest(kt[i], 3) for i in range(700)]))


# ---- 2. every measure on every path -----------------------------------------------------------------------------------
def datasets():
    n, L = 260, 3000
    r = synth.root(synth.SEED, L)
    low = synth.records(synth.SEED, r, 0, n)
    clade = low.copy()
    synth.apply_clades(clade, r, *synth.clade_plan(synth.SEED, n, L))
    nrun = low.copy()
    synth.apply_nruns(nrun, synth.nrun_plan(synth.SEED, n, L, share=0.1))
    return {"low": low, "clade": clade, "nrun": nrun, "uniform": uniform_codes(120, 64, seed=5)}


@pytest.fixture(scope="module")
def sets():
    return datasets()


@pytest.mark.parametrize("path", ["dense", "consensus", "hybrid"])
@pytest.mark.parametrize("kind", ["low", "clade", "nrun", "uniform"])
def test_every_measure_every_path(sets, path, kind):
    codes = sets[kind]
    n = len(codes)
    rng = np.random.default_rng(7)
    sample = rng.choice(n, 6, replace=False)
    with da.Engine(0) as eng:
        eng.set_prep_threshold(0)
        eng.set_path(path)
        eng.upload(0, codes)
        counts = eng.base_counts(0)
        for m in ALL:
            vals = eng.run_square(m)
            tal = eng.run_square(m, tallies=True)
            k = 9
            idx, got, gt = eng.nearest(m, k, tallies=True)
            assert np.array_equal(idx, expected_square(vals, n, k)), (path, kind, m)
            rows = np.repeat(np.arange(n), k).reshape(n, k)
            c = canon(n, rows, idx)
            assert np.array_equal(got.view(np.uint64), vals[c].view(np.uint64)), (path, kind, m)
            assert np.array_equal(gt, tal[c]), (path, kind, m)
            for i in sample:
                want = oracle.all_pairs_rect(m, codes[i:i + 1], codes)[0]
                for e in range(k):
                    j = int(idx[i, e])
                    q, t = min(i, j), max(i, j)
                    f = da.finalize(m, gt[i, e], counts[q], counts[t])
                    w = int(want[j]) if m in da.INT_MEASURES else float(want[j])
                    assert f == w or (f != f and w != w), (path, kind, m, i, j, f, w)


# ---- 3. ties -------------------------------------------------------------------------------------------------------------
def test_ties_in_index_order():
    base = random_alignment(5, 400, seed=31)
    codes = np.ascontiguousarray(base[np.arange(60) % 5])
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        for m in ("n_high", "raw", "tn93"):
            idx, vals = eng.nearest(m, 15)
            for i in range(60):
                copies = [j for j in range(i % 5, 60, 5) if j != i]
                assert list(idx[i, :11]) == copies, (m, i)
                assert np.all(vals[i, :11] == 0)
            assert np.array_equal(idx, expected_square(eng.run_square(m), 60, 15))


# ---- 4. many slabs -------------------------------------------------------------------------------------------------------
def expected_rect_rows(eng, measure, n_rows, k, exclude_diag, chunk=1000):
    out = []
    for rb in range(0, n_rows, chunk):
        re = min(n_rows, rb + chunk)
        kk = keys(eng.run_rect(measure, 0, 1, rb, re))
        out += [smallest(kk[r], k, exclude=(rb + r) if exclude_diag else -1) for r in range(re - rb)]
    return np.array(out)


def test_square_many_slabs():
    n = 12_000
    assert n * (n - 1) // 2 > 2 * SLAB_PAIRS
    codes = random_alignment(n, 200, seed=41)
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        idx, vals = eng.nearest("raw", 12)
        idx2, vals2 = eng.nearest("raw", 12)
        assert np.array_equal(idx, idx2) and np.array_equal(vals.view(np.uint64), vals2.view(np.uint64))
        eng.upload(1, codes)
        assert np.array_equal(idx, expected_rect_rows(eng, "raw", n, 12, True))


def test_rect_many_slabs():
    a = random_alignment(2_400, 150, seed=42)
    b = random_alignment(30_000, 150, seed=43)
    assert len(a) * len(b) > 2 * SLAB_PAIRS
    with da.Engine(0) as eng:
        eng.upload(0, a)
        eng.upload(1, b)
        idx, vals = eng.nearest("tn93", 10, square=False)
        idx2, vals2 = eng.nearest("tn93", 10, square=False)
        assert np.array_equal(idx, idx2) and np.array_equal(vals.view(np.uint64), vals2.view(np.uint64))
        assert np.array_equal(idx, expected_rect_rows(eng, "tn93", len(a), 10, False))


# ---- 5. state left behind ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["auto", "dense", "consensus"])
def test_run_square_unchanged(sets, path):
    codes = sets["nrun"]
    with da.Engine(0) as eng:
        eng.set_prep_threshold(0)
        eng.set_path(path)
        eng.upload(0, codes)
        for m in ("raw", "tn93"):
            before = eng.run_square(m)
            eng.nearest(m, 5)
            after = eng.run_square(m)
            assert np.array_equal(before.view(np.uint64), after.view(np.uint64)), (path, m)


# ---- 6. errors -----------------------------------------------------------------------------------------------------------
def test_errors():
    lib = da.load()
    codes = random_alignment(50, 100, seed=51)
    with da.Engine(0) as eng:
        h = eng._h
        eng.upload(0, codes)
        index = np.zeros(50 * 10, np.uint32)
        ku = C.c_uint32(99)

        def call(k, square=1, rs=0, cs=1, cap=500):
            return lib.dst_nearest(h, 2, square, rs, cs, k, index.ctypes.data, None, None, cap, C.byref(ku))

        assert call(0) == ERR_ARG and ku.value == 0
        assert call(257) == ERR_ARG
        assert call(10, cap=499) == ERR_CAPACITY
        assert call(10, square=0, rs=0, cs=1) == ERR_STATE      # slot 1 not uploaded
        assert call(10, square=0, rs=0, cs=0) == ERR_ARG        # one set: the square form
        assert lib.dst_nearest(h, 2, 1, 0, 0, 10, None, None, None, 500, C.byref(ku)) == ERR_ARG
        assert call(10) == 0 and ku.value == 10
        eng.upload(1, codes[:1])
        assert call(10, square=0, rs=0, cs=1, cap=50) == 0 and ku.value == 1
        assert np.all(index[:50] == 0)
    with da.Engine(0) as eng:
        eng.upload(0, codes[:1])
        idx, vals = eng.nearest("raw", 4)
        assert idx.shape == (1, 0)


# ---- 7. full size --------------------------------------------------------------------------------------------------------
def test_full_size_sampled_rows():
    n, L = 50_000, 30_000
    codes = synth.alignment(synth.SEED ^ 7, n, L)
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        idx, vals = eng.nearest("raw", 10)
    assert idx.shape == (n, 10)
    rows = np.random.default_rng(3).choice(n, 16, replace=False)
    rows[:2] = (0, n - 1)
    for i in rows:
        want = oracle.all_pairs_rect("raw", codes[i:i + 1], codes, threads=16)[0]
        exp = smallest(keys(want), 10, exclude=int(i))
        assert np.array_equal(idx[i], exp), i
        assert np.array_equal(vals[i].view(np.uint64), want[exp].view(np.uint64)), i


# ---- lists wider than one wave: 64 s + lane in slot s, carried across slots through lane 63 -> lane 0 -----------------
WIDE_K = (63, 64, 65, 127, 128, 129, 192, 193, 255, 256)


def tied_alignment(n, L, seed):
    """low diversity on a short alignment: a handful of distinct n_high values, so nearly every list boundary is a tie"""
    rng = np.random.default_rng(seed)
    root = rng.choice(np.array([136, 72, 40, 24], np.uint8), size=L)
    codes = np.tile(root, (n, 1))
    m = rng.random((n, L)) < 0.02
    codes[m] = rng.choice(np.array([136, 72, 40, 24, 240, 192], np.uint8), size=int(m.sum()))
    return codes


def sample_rows(n, n_cols, square, seed):
    """first and last rows, the rows either side of every slab cut, and a random few"""
    cuts, pairs = [], 0
    for i in range(n):
        w = n_cols - i - 1 if square else n_cols
        if pairs + w > SLAB_PAIRS:
            cuts += [i - 1, i]
            pairs = 0
        pairs += w
    rng = np.random.default_rng(seed)
    return sorted({0, 1, n - 2, n - 1, *cuts} | {int(x) for x in rng.integers(0, n, 40)}), len(cuts) // 2 + 1


@pytest.mark.parametrize("k", WIDE_K)
def test_wide_lists_with_heavy_ties_over_several_slabs(wide_engine, k):
    """square: the row pass and the column pass each merge into a record's list once per slab"""
    eng, codes = wide_engine
    n = len(codes)
    rows, slabs = sample_rows(n, n, True, k)
    assert slabs >= 3
    idx, vals = eng.nearest("n_high", k)
    assert idx.shape == (n, k)
    want = oracle.all_pairs_rect("n_high", codes[rows], codes, threads=16).astype(np.int64)
    kk = keys(want)
    for r, i in enumerate(rows):
        exp = smallest(kk[r], k, exclude=i)
        assert np.array_equal(idx[i], exp), (k, i)
        assert np.array_equal(vals[i], want[r][exp]), (k, i)
    # heavy ties, by the oracle's values: in most rows the last entry kept and the first one left out are equal
    tied = [np.sort(np.delete(want[r], i))[k - 1:k + 1] for r, i in enumerate(rows)]
    assert sum(int(a == b) for a, b in tied) > len(rows) // 2


@pytest.fixture(scope="module")
def wide_engine():
    codes = tied_alignment(12_500, 64, seed=81)
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        yield eng, codes


@pytest.fixture(scope="module")
def wide_rect_engine():
    a, b = tied_alignment(4200, 64, seed=82), tied_alignment(25_000, 64, seed=83)
    with da.Engine(0) as eng:
        eng.upload(0, a)
        eng.upload(1, b)
        yield eng, a, b


@pytest.mark.parametrize("k", WIDE_K)
def test_wide_lists_rectangle_over_several_slabs(wide_rect_engine, k):
    eng, a, b = wide_rect_engine
    rows, slabs = sample_rows(len(a), len(b), False, k)
    assert slabs >= 3
    idx, vals = eng.nearest("n_high", k, square=False, row_slot=0, col_slot=1)
    assert idx.shape == (len(a), k)
    want = oracle.all_pairs_rect("n_high", a[rows], b, threads=16).astype(np.int64)
    kk = keys(want)
    for r, i in enumerate(rows):
        exp = smallest(kk[r], k)
        assert np.array_equal(idx[i], exp), (k, i)
        assert np.array_equal(vals[i], want[r][exp]), (k, i)


def special_values_set():
    """40 x 400: ten copies of a root (zeros; jc69 / k80 give -0.0), ten records that differ from it at exactly 300 sites
    (raw 0.75: jc69 +inf), five records without a resolved site (raw NaN against everyone), fifteen ordinary ones"""
    rng = np.random.default_rng(91)
    L = 400
    root = rng.choice(np.array([136, 72, 40, 24], np.uint8), size=L)
    alt = np.array([{136: 72, 72: 136, 40: 24, 24: 40}[int(c)] for c in root], np.uint8)
    codes = np.tile(root, (40, 1))
    codes[10:20, :300] = alt[:300]
    codes[20:25] = 240
    m = rng.random((15, L)) < 0.05
    codes[25:][m] = rng.choice(np.array([136, 72, 40, 24], np.uint8), size=int(m.sum()))
    return codes


@pytest.mark.parametrize("path", ["dense", "consensus"])
def test_nan_inf_and_signed_zeros_inside_a_list(path):
    """k larger than the number of finite candidates: the infinities come after every finite value, the NaN block after
    them, each ordered by index; zeros of either sign tie and are ordered by index; every value comes back with the
    bits run_square gives that pair (a -0.0 stays -0.0); k_used is min(k, n - 1)"""
    codes = special_values_set()
    n = len(codes)
    with da.Engine(0) as eng:
        eng.set_prep_threshold(0)
        eng.set_path(path)
        eng.upload(0, codes)
        for m in ALL:
            if m in ("n", "n_high", "raw"):
                cond = as_payload(m, oracle.all_pairs_square(m, codes))
                assert np.array_equal(eng.run_square(m).view(np.uint64), cond.view(np.uint64)), m
            else:
                cond = eng.run_square(m)
            for k in (39, 64, 256):
                idx, vals = eng.nearest(m, k)
                assert idx.shape == (n, 39), (m, k)                        # k_used = n - 1
                assert np.array_equal(idx, expected_square(cond, n, 39)), (m, k)
                rows = np.repeat(np.arange(n), 39).reshape(n, 39)
                assert np.array_equal(vals.view(np.uint64), cond[canon(n, rows, idx)].view(np.uint64)), (m, k)
            if m in da.INT_MEASURES:
                continue
            # row 0 (a copy of the root), its blocks as the ORACLE's values say: zeros first, the infinities after every
            # finite value, the NaN block last, each in index order
            o = square_matrix(oracle.all_pairs_square(m, codes), n)[0]
            others = np.arange(1, n)
            zeros, infs, nans = (others[f(o[1:])] for f in (lambda x: x == 0, np.isposinf, np.isnan))
            v = vals[0]
            assert len(zeros) == 9 and len(nans) >= 5 and (m != "jc69" or len(infs) == 10), (m, zeros, infs, nans)
            assert (v[:9] == 0).all() and list(idx[0][:9]) == list(zeros), (m, v)
            assert np.isnan(v[39 - len(nans):]).all() and list(idx[0][39 - len(nans):]) == list(nans), (m, v)
            at = 39 - len(nans) - len(infs)
            assert np.isposinf(v[at:at + len(infs)]).all() and list(idx[0][at:at + len(infs)]) == list(infs), (m, v)
            assert np.isfinite(v[:at]).all()
            if m in ("jc69", "k80"):
                assert np.signbit(v[:9]).all() and np.signbit(o[zeros]).all()     # -k ln(1) = -0.0, and it stays -0.0
            assert np.isnan(vals[22]).all() and list(idx[22]) == [j for j in range(n) if j != 22], m
