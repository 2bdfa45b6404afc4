"""GPU (-m gpu): dst_run_windows / dst_window_base_counts against window_reference (the oracle on contiguous copies of the
column slices) and, bit for bit, against run_square / run_rect of a second context that holds the cut columns: window
edges, no leak across an edge, the table of all code pairs, tile edges, the grid limit, wide tallies, base counts, state,
capacity and errors.  Shapes are the smallest at which the kernel can go wrong."""
import ctypes as C

import numpy as np
import pytest

import distance_amd as da
import oracle
from helpers import CODES, KNOWN, random_alignment, uniform_codes
from tools import synth
from window_reference import ALL, WIDTH, expected_counts, expected_tallies, pair_index

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE, ERR_CAPACITY = 1, 4, 6
FLOAT = ("raw", "jc69", "k80", "tn93")
EDGES = (0, 1, 31, 32, 33, 127, 128, 129, 255, 256, 257)


@pytest.fixture(scope="module")
def eng():
    with da.Engine(0) as e:
        yield e


@pytest.fixture(scope="module")
def cut():
    """the context that holds a window's columns as a set of their own"""
    with da.Engine(0) as e:
        yield e


def edge_windows(length, seed):
    """every [b, e), b <= e, over the edge values clipped to `length`; one window repeated, the list shuffled"""
    edges = sorted({min(x, length) for x in EDGES + (length - 1, length)})
    wins = [(b, e) for b in edges for e in edges if b <= e]
    wins.append(wins[len(wins) // 2])
    rng = np.random.default_rng(seed)
    return np.array(wins, np.uint64)[rng.permutation(len(wins))]


def reference(measure, a, b, windows, square):
    """window_reference on the distinct windows only (the list repeats one)"""
    uniq, inv = np.unique(windows, axis=0, return_inverse=True)
    return expected_tallies(measure, a, b, uniq, square=square)[inv.reshape(-1)]


def same_bits(got, want):
    """equal bits, or both NaN"""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype.kind != "f":
        return got.dtype == want.dtype and np.array_equal(got, want)
    return got.shape == want.shape and bool(((got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))).all())


def zero_value(measure):
    """what the finalisation gives for an empty window"""
    z4 = np.zeros(4, np.uint32)
    return da.finalize(measure, np.zeros(WIDTH[measure], np.uint32), z4, z4)


# ---- window edges ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", ALL)
@pytest.mark.parametrize("n", [2, 3, 65, 257])
@pytest.mark.parametrize("length", [1, 127, 128, 129, 257, 1000])
def test_window_edges(eng, cut, length, n, measure):
    codes = uniform_codes(n, length, seed=1000 * n + length)
    codes[:, np.random.default_rng(n + length).random(length) < 0.4] = 136   # (so that windows differ in every tally)
    other = uniform_codes(3, length, seed=7 * n + length)
    windows = edge_windows(length, seed=n * length)
    nw = len(windows)
    empty = windows[:, 0] == windows[:, 1]
    assert empty.sum() >= 2 and (windows[:, 1] - windows[:, 0] == 1).any() and (windows == (0, length)).all(axis=1).any()
    eng.set_path("auto")
    eng.upload(0, codes)
    eng.upload(1, other)
    want_sq = reference(measure, codes, None, windows, True)
    i_all, _ = pair_index(True, n, n)
    # the square: tallies of every row range against the reference
    for rb, re in ((0, n), (1, n - 1), (n - 1, n), (1, 1)):
        keep = (i_all >= rb) & (i_all < re)
        tal = eng.run_windows(measure, windows, row_begin=rb, row_end=re, tallies=True)
        assert tal.dtype == np.uint32 and tal.shape == (nw, int(keep.sum()), WIDTH[measure]), (rb, re)
        assert np.array_equal(tal, want_sq[:, keep]), (measure, rb, re)
        val = eng.run_windows(measure, windows, row_begin=rb, row_end=re)
        assert val.shape == (nw, int(keep.sum())) and val.dtype == (np.float64 if measure in FLOAT else np.int64)
        if keep.any():
            assert same_bits(val[empty], np.full((int(empty.sum()), int(keep.sum())), zero_value(measure))), (measure, rb, re)
    # both rectangle orientations
    rect = {}
    for rs, cs, a, b in ((0, 1, codes, other), (1, 0, other, codes)):
        want = reference(measure, a, b, windows, False)
        tal = eng.run_windows(measure, windows, square=False, row_slot=rs, col_slot=cs, tallies=True)
        assert np.array_equal(tal, want), (measure, rs, cs)
        rows = a.shape[0]
        if rows > 2:   # a row range inside
            part = eng.run_windows(measure, windows, square=False, row_slot=rs, col_slot=cs, row_begin=1, row_end=rows - 1,
                                   tallies=True)
            assert np.array_equal(part, want.reshape(nw, rows, -1, WIDTH[measure])[:, 1:rows - 1].reshape(nw, -1, WIDTH[measure]))
        rect[(rs, cs)] = (tal, eng.run_windows(measure, windows, square=False, row_slot=rs, col_slot=cs))
    sq_tal, sq_val = eng.run_windows(measure, windows, tallies=True), eng.run_windows(measure, windows)
    # bit for bit what a context holding the cut columns returns, dense and on auto (at most 12 windows per shape)
    picked = [w for w in range(nw) if not empty[w]][:12]
    for w in picked:
        lo, hi = int(windows[w, 0]), int(windows[w, 1])
        cut.upload(0, np.ascontiguousarray(codes[:, lo:hi]))
        cut.upload(1, np.ascontiguousarray(other[:, lo:hi]))
        for path in ("dense", "auto"):
            cut.set_path(path)
            assert same_bits(sq_val[w], cut.run_square(measure)), (measure, w, path)
            assert np.array_equal(sq_tal[w], cut.run_square(measure, tallies=True).reshape(-1, WIDTH[measure])), (measure, w, path)
            for rs, cs in ((0, 1), (1, 0)):
                tal, val = rect[(rs, cs)]
                assert same_bits(val[w], cut.run_rect(measure, rs, cs).reshape(-1)), (measure, w, path, rs)
                assert np.array_equal(tal[w], cut.run_rect(measure, rs, cs, tallies=True).reshape(-1, WIDTH[measure]))


# ---- no leak across a window's edge ------------------------------------------------------------------------------------
def test_no_leak_across_an_edge(eng):
    """per window two pairs: equal inside and A against C at every site outside it, and the converse"""
    length, marks = 300, (1, 31, 32, 33, 127, 128, 129)
    windows = np.array([(b, e) for b in marks for e in marks if b <= e], np.uint64)
    nw = len(windows)
    rng = np.random.default_rng(5)
    codes = np.empty((4 * nw, length), np.uint8)
    for w, (b, e) in enumerate(windows.tolist()):
        inside = np.array(KNOWN, np.uint8)[rng.integers(0, 4, length)]
        p, q, r, s = codes[4 * w:4 * w + 4]
        p[:], q[:] = 136, 40            # equal inside, A against C outside
        p[b:e] = q[b:e] = inside[b:e]
        r[:] = s[:] = inside            # A against C inside, equal outside
        r[b:e], s[b:e] = 136, 40
    n = 4 * nw
    at = lambda i, j: i * (2 * n - i - 1) // 2 + (j - i - 1)   # noqa: E731
    eng.set_path("auto")
    eng.upload(0, codes)
    for m in ALL:
        tal = eng.run_windows(m, windows, tallies=True).astype(np.int64)
        val = eng.run_windows(m, windows)
        for w, (b, e) in enumerate(windows.tolist()):
            size = e - b
            same, diff = tal[w, at(4 * w, 4 * w + 1)], tal[w, at(4 * w + 2, 4 * w + 3)]
            want_same = {"n": [0], "n_high": [0], "raw": [0, size], "jc69": [0, size], "k80": [size, 0, 0], "tn93": [size, 0, 0, 0]}[m]
            want_diff = {"n": [size], "n_high": [size], "raw": [size, size], "jc69": [size, size], "k80": [size, 0, size],
                         "tn93": [size, size, 0, 0]}[m]
            assert same.tolist() == want_same and diff.tolist() == want_diff, (m, b, e)
            if m in ("n", "n_high"):
                assert val[w, at(4 * w, 4 * w + 1)] == 0 and val[w, at(4 * w + 2, 4 * w + 3)] == size
            elif m == "raw" and size:
                assert val[w, at(4 * w, 4 * w + 1)] == 0.0 and val[w, at(4 * w + 2, 4 * w + 3)] == 1.0


# ---- the table of all code pairs -----------------------------------------------------------------------------------------
def test_code_table(eng):
    """all 17 x 17 Paradis code pairs at sites 0, 31, 32, 127, 128 of a 200-site alignment, seen through one-site windows"""
    sites = (0, 31, 32, 127, 128)
    a, b = uniform_codes(17, 200, seed=3), uniform_codes(17, 200, seed=4)
    for s in sites:
        a[:, s] = CODES
        b[:, s] = CODES
    windows = np.array([(s, s + 1) for s in sites], np.uint64)
    lib = da.load()
    out = (C.c_int * 4)()
    eng.set_path("auto")
    eng.upload(0, a)
    eng.upload(1, b)
    for m in ALL:
        mid = lib.dst_measure_from_name(m.encode())
        want = np.zeros((17, 17, WIDTH[m]), np.uint32)
        for x in range(17):
            for y in range(17):
                assert lib.dst_site_tallies(mid, int(CODES[x]), int(CODES[y]), out) == 0
                want[x, y] = out[:WIDTH[m]]
        tal = eng.run_windows(m, windows, square=False, tallies=True).reshape(len(sites), 17, 17, WIDTH[m])
        for w in range(len(sites)):
            assert np.array_equal(tal[w], want), (m, sites[w])


# ---- tile edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cols", [255, 256, 257, 513])
def test_tile_edges(eng, n_cols):
    length = 64
    cols = uniform_codes(n_cols, length, seed=n_cols)
    windows = np.array([(0, 64), (5, 40), (63, 64)], np.uint64)
    eng.set_path("auto")
    eng.upload(0, cols)
    i_all, _ = pair_index(True, n_cols, n_cols)
    for m in ("n", "raw", "k80", "tn93"):
        want = expected_tallies(m, cols, None, windows, square=True)
        for rb, re in ((0, 1), (0, 9), (n_cols - 9, n_cols), (250, 259)):
            re = min(re, n_cols)
            keep = (i_all >= rb) & (i_all < re)
            assert np.array_equal(eng.run_windows(m, windows, row_begin=rb, row_end=re, tallies=True), want[:, keep]), (m, rb, re)
    for n_rows in (1, 9):
        rows = uniform_codes(n_rows, length, seed=100 + n_rows)
        eng.upload(1, rows)
        for m in ("n", "raw", "k80", "tn93"):
            want = expected_tallies(m, rows, cols, windows)
            assert np.array_equal(eng.run_windows(m, windows, square=False, row_slot=1, col_slot=0, tallies=True), want), (m, n_rows)
            want = expected_tallies(m, cols, rows, windows)   # (and the few records on the lanes)
            assert np.array_equal(eng.run_windows(m, windows, square=False, row_slot=0, col_slot=1, tallies=True), want), (m, n_rows)


# ---- the grid limit ----------------------------------------------------------------------------------------------------------
def test_65536_windows(eng):
    """exactly the maximum: more windows than one grid axis holds; one more is refused"""
    length = 300
    codes = uniform_codes(2, length, seed=9)
    rng = np.random.default_rng(9)
    pool_b = rng.integers(0, length + 1, 3000)
    pool = np.stack([pool_b, pool_b + rng.integers(0, length + 1 - pool_b)], axis=1).astype(np.uint64)
    ones = np.stack([np.arange(length), np.arange(length) + 1], axis=1).astype(np.uint64)
    windows = np.concatenate([ones, pool[rng.integers(0, len(pool), da.WINDOWS_MAX - length)]])
    assert len(windows) == da.WINDOWS_MAX == 65536
    eng.set_path("auto")
    eng.upload(0, codes)
    for m in ("raw", "tn93"):
        got = eng.run_windows(m, windows, tallies=True)
        assert got.shape == (65536, 1, WIDTH[m])
        assert np.array_equal(got, reference(m, codes, None, windows, True)), m
    val = eng.run_windows("n", windows)
    assert np.array_equal(val[:, 0], reference("n", codes, None, windows, True)[:, 0, 0].astype(np.int64))
    uniq, inv = np.unique(windows, axis=0, return_inverse=True)
    assert np.array_equal(eng.window_base_counts(0, windows), expected_counts(codes, uniq)[inv.reshape(-1)])
    with pytest.raises(da.DistanceError) as e:
        eng.run_windows("n", np.concatenate([windows, windows[:1]]))
    assert e.value.status == ERR_ARG and "65,536" in e.value.message


# ---- wide tallies ------------------------------------------------------------------------------------------------------------
def test_wide_tallies(eng):
    """2 records that differ at every one of 70,000 sites: tallies past 16 bits"""
    length = 70_000
    codes = np.empty((2, length), np.uint8)
    codes[0], codes[1] = 136, 40
    windows = np.array([(0, length), (1, length - 1)], np.uint64)
    eng.set_path("auto")
    eng.upload(0, codes)
    assert eng.run_windows("n", windows)[:, 0].tolist() == [70_000, 69_998]
    assert eng.run_windows("n_high", windows, tallies=True)[:, 0, 0].tolist() == [70_000, 69_998]
    assert eng.run_windows("raw", windows, tallies=True)[:, 0].tolist() == [[70_000, 70_000], [69_998, 69_998]]
    assert eng.run_windows("k80", windows, tallies=True)[:, 0].tolist() == [[70_000, 0, 70_000], [69_998, 0, 69_998]]
    assert eng.run_windows("tn93", windows, tallies=True)[:, 0].tolist() == [[70_000, 70_000, 0, 0], [69_998, 69_998, 0, 0]]
    assert eng.run_windows("raw", windows)[:, 0].tolist() == [1.0, 1.0]
    for m in ALL:
        assert np.array_equal(eng.run_windows(m, windows, tallies=True), expected_tallies(m, codes, None, windows, square=True)), m


# ---- base counts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [1, 127, 128, 129, 257, 1000])
def test_base_counts(eng, length):
    n = 67
    codes = random_alignment(n, length, seed=length, p_ambig=0.1, p_gap=0.1, divergence=0.2)   # (ambiguity codes, N, - and ?)
    other = random_alignment(3, length, seed=length + 1, p_ambig=0.1, p_gap=0.1, divergence=0.2, root=codes[0])
    assert all((codes == c).any() for c in CODES) or length < 300
    windows = edge_windows(length, seed=length)
    uniq, inv = np.unique(windows, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    eng.set_path("auto")
    eng.upload(0, codes)
    eng.upload(1, other)
    qc, tc = eng.window_base_counts(0, windows), eng.window_base_counts(1, windows)
    assert qc.dtype == np.uint32 and qc.shape == (len(windows), n, 4) and tc.shape == (len(windows), 3, 4)
    assert np.array_equal(qc, expected_counts(codes, uniq)[inv]) and np.array_equal(tc, expected_counts(other, uniq)[inv])
    # tn93: tallies + these counts + the host's finalisation = the oracle's distance on the cut columns, bit for bit
    tal = eng.run_windows("tn93", windows, square=False, tallies=True)
    for w in range(0, len(windows), 5):
        lo, hi = int(windows[w, 0]), int(windows[w, 1])
        if hi == lo:
            continue
        a, b = np.ascontiguousarray(codes[:, lo:hi]), np.ascontiguousarray(other[:, lo:hi])
        want = oracle.all_pairs_rect("tn93", a, b, oracle.count_bases_matrix(a), oracle.count_bases_matrix(b)).reshape(-1)
        got = np.array([da.finalize("tn93", tal[w, p], qc[w, p // 3], tc[w, p % 3]) for p in range(n * 3)])
        assert same_bits(got, want), (length, lo, hi)


# ---- state ---------------------------------------------------------------------------------------------------------------------
def test_deferred_planes_and_untouched_state():
    n, length = 1100, 3333
    rng = np.random.default_rng(31)
    codes = synth.alignment(synth.SEED ^ 31, n, length)
    for r in rng.choice(n, 50, replace=False):
        at = rng.choice(length, 20, replace=False)
        codes[r, at] = CODES[rng.integers(0, 17, len(at))]
    windows = np.array([(0, length), (100, 1100), (127, 129), (3332, 3333), (500, 500)], np.uint64)
    with da.Engine(0) as dense, da.Engine(0) as lazy:
        dense.set_path("dense")
        dense.upload(0, codes)
        assert dense.planes_stored(0)
        lazy.set_prep_threshold(0)
        lazy.upload(0, codes)
        assert not lazy.planes_stored(0), "the upload stored every plane: nothing here tests the deferred form"
        lazy.set_path("consensus")
        before = {m: lazy.run_square(m, 0, 40) for m in ("n", "tn93")}
        launch, path = lazy.last_launch(), lazy.last_path()
        assert not lazy.planes_stored(0)
        for m in ALL:
            for tallies in (True, False):
                got = lazy.run_windows(m, windows, row_begin=3, row_end=30, tallies=tallies)
                want = dense.run_windows(m, windows, row_begin=3, row_end=30, tallies=tallies)
                assert same_bits(got, want), (m, tallies)
            assert lazy.planes_stored(0)
            assert lazy.last_launch() == launch and lazy.last_path() == path, m
        part = lazy.run_windows("raw", windows[:2], row_begin=3, row_end=5, tallies=True)
        assert np.array_equal(part, expected_tallies("raw", codes, None, windows[:2], square=True, rb=3, re=5))
        assert np.array_equal(lazy.window_base_counts(0, windows), dense.window_base_counts(0, windows))
        for m, v in before.items():
            assert lazy.run_square(m, 0, 40).tobytes() == v.tobytes() and lazy.last_path() == "consensus", m
            assert same_bits(dense.run_square(m, 0, 40), v), m


class Hip:
    """device memory and a stream without torch"""

    def __init__(self):
        self.lib = C.CDLL("libamdhip64.so")
        self.lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.lib.hipFree.argtypes = [C.c_void_p]
        self.lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.lib.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        self.lib.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
        self.lib.hipStreamDestroy.argtypes = [C.c_void_p]

    def malloc(self, nbytes):
        p = C.c_void_p()
        assert self.lib.hipMalloc(C.byref(p), nbytes) == 0
        assert self.lib.hipMemset(p, 0, nbytes) == 0 and self.lib.hipDeviceSynchronize() == 0
        return p.value

    def to_device(self, a):
        p = self.malloc(a.nbytes)
        assert self.lib.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
        return p

    def to_host(self, p, dtype, count):
        out = np.zeros(count, dtype)
        assert self.lib.hipDeviceSynchronize() == 0 and self.lib.hipMemcpy(out.ctypes.data, p, out.nbytes, 2) == 0
        return out


def test_shared_set_is_refused():
    from shared_ranks import ThreadRanks
    n, length = 2_500, 3_000   # (a shape of test_gpu_shared: the lists fit their blocks, no rank falls back to a full upload)
    codes = synth.alignment(synth.SEED ^ 9, n, length)
    hip = Hip()
    d_codes = hip.to_device(codes)
    windows = np.array([(0, 100)], np.uint64)

    def body(rank, eng, comm):
        eng.upload_shared(comm, 0, d_codes, n, length, length, with_counts=True)
        assert eng.shared_stats()["fallbacks"] == 0
        out = []
        for call in (lambda: eng.run_windows("raw", windows, row_begin=0, row_end=2),
                     lambda: eng.window_base_counts(0, windows)):
            with pytest.raises(da.DistanceError) as e:
                call()
            out.append((e.value.status, e.value.message))
        return out

    try:
        for res in ThreadRanks(2).run(body):
            for status, message in res:
                assert status == ERR_STATE and "dst_upload_shared runs on the consensus path only" in message
    finally:
        hip.lib.hipFree(d_codes)


# ---- capacity and errors -----------------------------------------------------------------------------------------------------
def test_capacity_and_errors():
    codes = uniform_codes(9, 200, seed=5)
    windows = np.array([(0, 200), (10, 20), (199, 200)], np.uint64)
    lib = da.load()
    guard = 64
    with da.Engine(0) as eng:
        h = eng._h

        def call(measure=2, square=1, rs=0, cs=1, rb=0, re=9, wb=windows[:, 0], we=windows[:, 1], nw=3, kind=1, cap=None, out=True):
            P, width = 36 if square else (re - rb) * 9, 2
            need = nw * P * width * 4 if kind == 1 else nw * P * 8
            buf = np.full(need + 2 * guard, 0xAB, np.uint8)
            wb = None if wb is None else np.ascontiguousarray(wb)
            we = None if we is None else np.ascontiguousarray(we)
            rc = lib.dst_run_windows_host(h, measure, square, rs, cs, rb, re, None if wb is None else wb.ctypes.data,
                                          None if we is None else we.ctypes.data, nw, kind, buf.ctypes.data + guard if out else None,
                                          need if cap is None else cap)
            return rc, buf, need, eng._lib.dst_last_error(h).decode()

        rc, _, _, msg = call()
        assert rc == ERR_STATE and msg == "set not uploaded"
        eng.upload(0, codes)
        want = expected_tallies("raw", codes, None, windows, square=True)
        rc, buf, need, _ = call()
        assert rc == 0 and np.array_equal(buf[guard:guard + need].view(np.uint32).reshape(3, 36, 2), want)
        assert (buf[:guard] == 0xAB).all() and (buf[guard + need:] == 0xAB).all()
        rc, buf, need, msg = call(cap=need - 1)
        assert rc == ERR_CAPACITY and (buf == 0xAB).all() and "too small" in msg
        rc, buf, need, _ = call(kind=0)
        assert rc == 0 and (buf[guard + need:] == 0xAB).all()
        rc, buf, need, _ = call(kind=0, cap=3 * 36 * 8 - 1)
        assert rc == ERR_CAPACITY and (buf == 0xAB).all()
        # DST_OK, nothing written: no window, an empty row range
        for kw in (dict(nw=0), dict(rb=4, re=4), dict(rb=8, re=9)):
            rc, buf, _, _ = call(**kw)
            assert rc == 0 and (buf == 0xAB).all(), kw
        bad = [
            (dict(measure=6), "unknown measure"), (dict(measure=-1), "unknown measure"),
            (dict(kind=2), "DST_OUT_TALLY16"), (dict(kind=3), "unknown output kind"),
            (dict(wb=None), "null pointer"), (dict(we=None), "null pointer"), (dict(out=False), "null output pointer"),
            (dict(rb=5, re=4), "row range out of bounds"), (dict(re=10), "row range out of bounds"),
            (dict(wb=np.array([0, 21, 5], np.uint64)), "window 1 [21, 20)"),
            (dict(we=np.array([200, 20, 201], np.uint64)), "window 2 [199, 201)"),
            (dict(square=0, rs=0, cs=0), "row_slot == col_slot"), (dict(square=0, rs=0, cs=2), "slot must be 0 or 1"),
            (dict(square=0, rs=-1, cs=0), "slot must be 0 or 1"),
        ]
        for kw, text in bad:
            rc, buf, _, msg = call(**kw)
            assert rc == ERR_ARG and text in msg and (buf == 0xAB).all(), (kw, rc, msg)
        rc, _, _, msg = call(square=0, rs=0, cs=1)
        assert rc == ERR_STATE and msg == "set not uploaded"
        eng.upload(1, uniform_codes(5, 90, seed=6))
        rc, _, _, msg = call(square=0, rs=0, cs=1)
        assert rc == ERR_STATE and "Different length sequences" in msg
        # the device form: the same checks, and a result on the caller's stream
        assert lib.dst_run_windows(h, 2, 1, 0, 1, 0, 9, windows[:, 0].copy().ctypes.data, windows[:, 1].copy().ctypes.data, 3, 1,
                                   None, 3 * 36 * 8, None) == ERR_ARG
        # dst_window_base_counts
        wb, we = np.ascontiguousarray(windows[:, 0]), np.ascontiguousarray(windows[:, 1])
        out = np.full(3 * 9 * 4 + 8, 0xABABABAB, np.uint32)
        assert lib.dst_window_base_counts(h, 0, wb.ctypes.data, we.ctypes.data, 3, out.ctypes.data, 3 * 9 * 4 - 1) == ERR_CAPACITY
        assert (out == 0xABABABAB).all()
        assert lib.dst_window_base_counts(h, 0, wb.ctypes.data, we.ctypes.data, 3, out.ctypes.data, 3 * 9 * 4) == 0
        assert np.array_equal(out[:108].reshape(3, 9, 4), expected_counts(codes, windows)) and (out[108:] == 0xABABABAB).all()
        assert lib.dst_window_base_counts(h, 2, wb.ctypes.data, we.ctypes.data, 3, out.ctypes.data, 200) == ERR_ARG
        assert lib.dst_window_base_counts(h, 0, None, we.ctypes.data, 3, out.ctypes.data, 200) == ERR_ARG
        assert lib.dst_window_base_counts(h, 0, wb.ctypes.data, we.ctypes.data, 3, None, 200) == ERR_ARG
        assert lib.dst_window_base_counts(h, 1, wb.ctypes.data, we.ctypes.data, 3, out.ctypes.data, 200) == ERR_ARG   # 200 > 90 sites
        assert "window 0 [0, 200)" in eng._lib.dst_last_error(h).decode()
        assert lib.dst_window_base_counts(h, 0, wb.ctypes.data, we.ctypes.data, da.WINDOWS_MAX + 1, out.ctypes.data, 200) == ERR_ARG
        # after the errors the context still answers
        assert np.array_equal(eng.run_windows("raw", windows, tallies=True), want)


def test_device_form_on_a_stream():
    """dst_run_windows into device memory, on the caller's stream and on the context's"""
    hip = Hip()
    codes = uniform_codes(70, 300, seed=8)
    windows = np.array([(0, 300), (31, 129), (128, 128)], np.uint64)
    wb, we = np.ascontiguousarray(windows[:, 0]), np.ascontiguousarray(windows[:, 1])
    lib = da.load()
    with da.Engine(0) as eng:
        eng.upload(0, codes)
        want_t, want_v = eng.run_windows("tn93", windows, tallies=True), eng.run_windows("tn93", windows)
        P = want_v.shape[1]
        stream = C.c_void_p()
        assert hip.lib.hipStreamCreate(C.byref(stream)) == 0
        for handle in (None, stream):
            d_t, d_v = hip.malloc(3 * P * 16), hip.malloc(3 * P * 8)
            assert lib.dst_run_windows(eng._h, 5, 1, 0, 1, 0, 70, wb.ctypes.data, we.ctypes.data, 3, 1, d_t, 3 * P * 16, handle) == 0
            assert lib.dst_run_windows(eng._h, 5, 1, 0, 1, 0, 70, wb.ctypes.data, we.ctypes.data, 3, 0, d_v, 3 * P * 8, handle) == 0
            assert np.array_equal(hip.to_host(d_t, np.uint32, 3 * P * 4).reshape(3, P, 4), want_t)
            assert same_bits(hip.to_host(d_v, np.float64, 3 * P).reshape(3, P), want_v)
            hip.lib.hipFree(d_t)
            hip.lib.hipFree(d_v)
        assert hip.lib.hipStreamDestroy(stream) == 0
