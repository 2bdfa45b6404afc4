"""GPU (-m gpu): dst_clusters / Engine.clusters, single-linkage clusters of one set — exact against a host union-find over
the links taken from the context's own run_square values, on every measure and kernel path, across row slabs, on
adversarial graphs (a permuted chain, a star), with NaN values, tiny sets, every error status, and at full size."""
import ctypes as C

import numpy as np
import pytest

import distance_amd as da
from helpers import KNOWN, random_alignment, uniform_codes
from tools import synth

pytestmark = pytest.mark.gpu
ALL = ("n", "n_high", "raw", "jc69", "k80", "tn93")
ERR_ARG, ERR_STATE, ERR_CAPACITY = 1, 4, 6
INF = float("inf")


# ---- the host reference -------------------------------------------------------------------------------------------------
def linked(measure, vals, threshold):
    """The documented link rule on DST_OUT_DISTANCE payloads: int64 v <= floor(T); f64 IEEE v <= T (NaN never)."""
    if measure in da.INT_MEASURES:
        f = np.floor(threshold)
        if f < -2.0 ** 63:
            return np.zeros(len(vals), bool)
        return vals <= (np.iinfo(np.int64).max if f >= 2.0 ** 63 else np.int64(f))
    with np.errstate(invalid="ignore"):
        return vals <= threshold


def components(n, a, b):
    """Labels of the connected components of the edges (a, b): the smallest record of each (union-find by hooking the
    larger root under the smallest proposed one, then pointer jumping, until every edge lies inside one tree)."""
    parent = np.arange(n, dtype=np.int64)
    a = np.asarray(a, np.int64)
    b = np.asarray(b, np.int64)
    while True:
        while True:
            nxt = parent[parent]
            if np.array_equal(nxt, parent):
                break
            parent = nxt
        ra, rb = parent[a], parent[b]
        cross = ra != rb
        if not cross.any():
            return parent.astype(np.uint32)
        lo, hi = np.minimum(ra[cross], rb[cross]), np.maximum(ra[cross], rb[cross])
        np.minimum.at(parent, hi, lo)
        a, b = a[cross], b[cross]


def pairs_of(n):
    return np.triu_indices(n, 1)


def reference(measure, vals, n, threshold):
    """(labels, links) from the condensed canonical-order square result."""
    link = linked(measure, vals, threshold)
    i, j = pairs_of(n)
    return components(n, i[link], j[link]), int(link.sum())


def interior(measure, vals):
    """A threshold inside the values: a small quantile of the finite ones (a few per cent of the pairs linked)."""
    v = vals[np.isfinite(vals)] if vals.dtype == np.float64 else vals
    return float(np.quantile(v, 0.02)) if len(v) else 0.0


# ---- 1. every measure on every path -------------------------------------------------------------------------------------
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
    with da.Engine(0) as eng:
        eng.set_prep_threshold(0)
        eng.set_path(path)
        eng.upload(0, codes)
        for m in ALL:
            vals = eng.run_square(m)
            for t in (0.0, interior(m, vals), INF):
                want, want_links = reference(m, vals, n, t)
                got, links = eng.clusters(m, t)
                assert got.dtype == np.uint32 and got.shape == (n,)
                assert np.array_equal(got, want), (path, kind, m, t)
                assert links == want_links, (path, kind, m, t)


# ---- 2. the slab bound does not change the result ----------------------------------------------------------------------
def test_slab_sizes(sets):
    codes = sets["clade"]
    n = len(codes)
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        for m in ("n_high", "raw", "tn93"):
            vals = eng.run_square(m)
            t = interior(m, vals)
            want = reference(m, vals, n, t)
            for max_pairs in (1, n - 1, 3000, 0):   # one row per slab (1: the bound is below a row), a few thousand, default
                got, links = eng.clusters(m, t, max_pairs=max_pairs)
                assert np.array_equal(got, want[0]) and links == want[1], (m, max_pairs)


def test_integer_threshold_is_floored(sets):
    codes = sets["low"]
    n = len(codes)
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        for m in ("n", "n_high"):
            vals = eng.run_square(m)
            t = float(np.quantile(vals, 0.05))
            a = eng.clusters(m, t)
            b = eng.clusters(m, t + 0.75)
            assert np.array_equal(a[0], b[0]) and a[1] == b[1]
            assert np.array_equal(a[0], reference(m, vals, n, t)[0])
            for neg in (-0.5, -1e300, -INF):   # floor(T) < 0: nothing links (every count is >= 0)
                got, links = eng.clusters(m, neg)
                assert links == 0 and np.array_equal(got, np.arange(n, dtype=np.uint32)), (m, neg)
            got, links = eng.clusters(m, 1e300)   # clamped to the int64 range: everything links
            assert links == n * (n - 1) // 2 and not got.any()


# ---- 3. adversarial graphs ---------------------------------------------------------------------------------------------
def chain_codes(n, seed):
    """Record perm[k] = the root with sites 0..k-1 changed: consecutive records of the chain are one site apart, any other
    two records at least two."""
    rng = np.random.default_rng(seed)
    root = rng.choice(np.array(KNOWN, np.uint8), size=n)
    other = np.array([KNOWN[(KNOWN.index(int(c)) + 1) % 4] for c in root], np.uint8)
    steps = np.tile(root, (n, 1))
    for k in range(n):
        steps[k, :k] = other[:k]
    perm = rng.permutation(n)
    codes = np.empty_like(steps)
    codes[perm] = steps
    return np.ascontiguousarray(codes), perm


def test_permuted_chain():
    n = 1500
    codes, perm = chain_codes(n, seed=71)
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        assert np.array_equal(eng.clusters("n_high", 1)[0], np.zeros(n, np.uint32))
        for max_pairs in (1, 2000, 0):
            for m, t in (("n_high", 1.5), ("n", 1.0), ("raw", 1.5 / n)):
                got, links = eng.clusters(m, t, max_pairs=max_pairs)
                assert links == n - 1, (m, max_pairs)
                assert np.array_equal(got, np.zeros(n, np.uint32)), (m, max_pairs)
        # two chains: positions n // 2 .. n-1 also differ at site n-1, so positions n // 2 - 1 and n // 2 are two apart
        codes2 = codes.copy()
        top = perm[n // 2:]
        codes2[top, n - 1] = KNOWN[(KNOWN.index(int(codes[top[0], n - 1])) + 1) % 4]
        eng.upload(0, codes2)
        want = np.empty(n, np.uint32)
        want[perm[:n // 2]] = perm[:n // 2].min()
        want[top] = top.min()
        for max_pairs in (1, 700, 0):
            got, links = eng.clusters("n_high", 1.0, max_pairs=max_pairs)
            assert links == n - 2 and np.array_equal(got, want), max_pairs
        vals = eng.run_square("n_high")
        assert np.array_equal(reference("n_high", vals, n, 1.0)[0], want)


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
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        for max_pairs in (1, 5000, 0):
            got, links = eng.clusters("n_high", 1, max_pairs=max_pairs)
            assert links == n - 1 and np.array_equal(got, np.zeros(n, np.uint32)), max_pairs
            got, links = eng.clusters("n_high", 0.5, max_pairs=max_pairs)
            assert links == 0 and np.array_equal(got, np.arange(n, dtype=np.uint32))
            got, links = eng.clusters("n_high", 2, max_pairs=max_pairs)
            assert links == n * (n - 1) // 2 and not got.any()


# ---- 4. NaN never links ------------------------------------------------------------------------------------------------
def test_nan_never_links():
    codes = uniform_codes(150, 40, seed=73)   # high divergence: jc69 / k80 / tn93 are NaN for many pairs
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        for m in ("jc69", "k80", "tn93"):
            vals = eng.run_square(m)
            nan = np.isnan(vals)
            assert nan.any(), m
            got, links = eng.clusters(m, INF)
            assert links == int((~nan).sum()), m
            assert np.array_equal(got, reference(m, vals, 150, INF)[0]), m
            got, links = eng.clusters(m, -0.0)   # -0.0 links wherever +0.0 does
            want = reference(m, vals, 150, 0.0)
            assert np.array_equal(got, want[0]) and links == want[1], m


# ---- 5. tiny sets, errors, state left behind ---------------------------------------------------------------------------
def test_tiny_sets():
    codes = random_alignment(3, 50, seed=74)
    with da.Engine(0) as eng:
        with pytest.raises(da.DistanceError):
            eng.upload(0, codes[:0])   # an empty set is not accepted by upload
        eng.upload(0, codes[:1])
        got, links = eng.clusters("raw", INF)
        assert list(got) == [0] and links == 0
        eng.upload(0, np.ascontiguousarray(codes[[0, 0]]))
        got, links = eng.clusters("raw", 0.0)
        assert list(got) == [0, 0] and links == 1
        eng.upload(0, codes[:2])
        got, links = eng.clusters("n_high", -1)
        assert list(got) == [0, 1] and links == 0


def test_errors():
    lib = da.load()
    codes = random_alignment(50, 100, seed=75)
    label = np.zeros(50, np.uint32)
    nc, nl = C.c_uint64(7), C.c_uint64(7)
    with da.Engine(0) as eng:
        h = eng._h
        assert lib.dst_clusters(h, 2, 1.0, 0, label.ctypes.data, 50, C.byref(nc), C.byref(nl)) == ERR_STATE
        eng.upload(0, codes)
        assert lib.dst_clusters(h, 2, float("nan"), 0, label.ctypes.data, 50, C.byref(nc), C.byref(nl)) == ERR_ARG
        assert lib.dst_clusters(h, 9, 1.0, 0, label.ctypes.data, 50, C.byref(nc), C.byref(nl)) == ERR_ARG
        assert lib.dst_clusters(h, -1, 1.0, 0, label.ctypes.data, 50, C.byref(nc), C.byref(nl)) == ERR_ARG
        assert lib.dst_clusters(h, 2, 1.0, 0, None, 50, C.byref(nc), C.byref(nl)) == ERR_ARG
        assert lib.dst_clusters(h, 2, 1.0, 0, label.ctypes.data, 49, C.byref(nc), C.byref(nl)) == ERR_CAPACITY
        assert lib.dst_clusters(h, 2, INF, 0, label.ctypes.data, 50, C.byref(nc), C.byref(nl)) == 0
        assert nc.value == 1 and nl.value == 50 * 49 // 2 and not label.any()
        assert lib.dst_clusters(h, 2, -1.0, 0, label.ctypes.data, 50, None, None) == 0
        assert np.array_equal(label, np.arange(50, dtype=np.uint32))
        assert lib.dst_clusters(h, 2, -1.0, 0, label.ctypes.data, 50, C.byref(nc), C.byref(nl)) == 0
        assert nc.value == 50 and nl.value == 0


@pytest.mark.parametrize("path", ["auto", "dense", "consensus"])
def test_run_square_unchanged(sets, path):
    codes = sets["nrun"]
    with da.Engine(0) as eng:
        eng.set_prep_threshold(0)
        eng.set_path(path)
        eng.upload(0, codes)
        for m in ("raw", "tn93"):
            before = eng.run_square(m)
            eng.clusters(m, interior(m, before), max_pairs=2000)
            after = eng.run_square(m)
            assert np.array_equal(before.view(np.uint64), after.view(np.uint64)), (path, m)


# ---- 6. full size ------------------------------------------------------------------------------------------------------
def test_full_size_sparse():
    n, L = 50_000, 30_000
    codes = synth.alignment(synth.SEED ^ 7, n, L)
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        # a sparse threshold: the 1e-4 quantile of a sample of rows (each row's own record left out)
        eng.upload(1, codes[::997])
        sample = eng.run_rect("raw", 1, 0)
        sample[np.arange(len(sample)), np.arange(0, n, 997)] = np.inf
        t = float(np.quantile(sample[np.isfinite(sample)], 1e-4))
        got, links = eng.clusters("raw", t)
        a_parts, b_parts = [], []

        def sink(first, rb, re, arr):
            # rows rb .. re-1 of the triangle, in canonical order
            hit = np.nonzero(arr <= t)[0].astype(np.int64)
            if len(hit):
                starts = np.array([i * (2 * n - i - 1) // 2 for i in range(rb, re + 1)], np.int64) - first
                row = np.searchsorted(starts, hit, side="right") - 1
                i = rb + row
                a_parts.append(i)
                b_parts.append(i + 1 + hit - starts[row])
            return False

        eng.run_slabs("raw", sink, 1 << 26)
    a = np.concatenate(a_parts) if a_parts else np.zeros(0, np.int64)
    b = np.concatenate(b_parts) if b_parts else np.zeros(0, np.int64)
    assert links == len(a) and links > 0
    assert np.array_equal(got, components(n, a, b))
    assert len(np.unique(got)) < n
