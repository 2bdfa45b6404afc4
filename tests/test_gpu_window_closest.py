"""GPU (-m gpu): window-closest streams (dst_stream_open_window_closest / Engine.window_closest_stream) — per (loaded record,
window) the k nearest streamed records, kept on the GPU while the stream goes past — bit for bit against the engine's own
nearest_windows and window_base_counts on the whole stream uploaded to slot 1, and for n / raw against the numpy
restatement of the definition: every measure, the row tile's and the list slots' boundaries, every cut, depth and wire,
every range cut, snapshots, other window calls in between, deferred planes, the ends of the ordinal range, and the errors."""
import ctypes as C

import numpy as np
import pytest

import distance_amd as da
from distance_amd import _lib
from helpers import CODES
from tools import synth
from window_closest_cases import CUTS, LOADED_SIZES, MAX_RECORDS, N_STREAMED, TIE_CUT, WINDOWS, loaded_set, reference, streamed_set
from window_nearest_reference import take

pytestmark = pytest.mark.gpu
ALL = ("n", "n_high", "raw", "jc69", "k80", "tn93")
KS = (1, 3, 64, 65, 256)            # the slot boundaries of the wave-resident list
ERR_ARG, ERR_INVALID_CODE, ERR_STATE, ERR_NOMEM, ERR_CAPACITY = 1, 3, 4, 5, 6
NW = len(WINDOWS)


@pytest.fixture(scope="module")
def eng():
    e = da.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def data():
    return loaded_set(), streamed_set()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype.itemsize == 8 else a


def assert_same(got, want, what=None):
    assert len(got) == len(want), what
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(bits(g), bits(w)), what


def status_of(fn, *a, **kw):
    with pytest.raises(da.DistanceError) as e:
        fn(*a, **kw)
    return e.value.status


def run_stream(eng, measure, k, streamed, cut, max_records=MAX_RECORDS, depth=3, nibbles=False, max_entries=0, windows=WINDOWS,
               first_index=None):
    """(index, values, tallies[, counts]) of the whole stream pushed in the batches of `cut`, depth - 1 in flight"""
    with eng.window_closest_stream(measure, windows, k, max_records, depth=depth, nibbles=nibbles, max_entries=max_entries) as st:
        if first_index is not None:
            st.next_index(first_index)
        at = 0
        for n in cut:
            if st.in_flight() == depth - 1:
                st.pop()
            st.push(streamed[at:at + n])
            at += n
        while st.in_flight():
            st.pop()
        return st.result(tallies=True, counts=measure == "tn93")


_want = {}


def yardstick(eng, measure, n_loaded, k, streamed, windows=WINDOWS, tag="set"):
    """What the definition names: nearest_windows(square=False) of slot 0 against the whole stream in slot 1, and for tn93 the
    listed records' window_base_counts.  Computed once per case and never changed; slot 0 must hold the loaded set."""
    key = (tag, measure, n_loaded, k)
    if key not in _want:
        eng.upload(1, streamed)
        idx, vals, tal = eng.nearest_windows(measure, windows, k, square=False, tallies=True)
        out = (idx, vals, tal)
        if measure == "tn93":
            cnt = eng.window_base_counts(1, windows)                 # (n_windows, n_streamed, 4)
            out += (cnt[np.arange(len(windows))[None, :, None], idx.astype(np.int64)],)
        _want[key] = out
    return _want[key]


# ---- 1. every measure, the row tile's boundary, k at the slot boundaries ----------------------------------------------------
@pytest.mark.parametrize("measure", ALL)
@pytest.mark.parametrize("n_loaded", LOADED_SIZES)
def test_every_measure_size_and_k(eng, data, n_loaded, measure):
    loaded, streamed = data[0][:n_loaded], data[1]
    eng.upload(0, loaded)
    for k in KS:
        want = yardstick(eng, measure, n_loaded, k, streamed)
        got = run_stream(eng, measure, k, streamed, TIE_CUT)
        assert got[0].shape == (n_loaded, NW, k) and got[0].dtype == np.uint32
        assert got[1].dtype == (np.int64 if measure in da.INT_MEASURES else np.float64)
        assert_same(got, want, (measure, n_loaded, k))
        if measure == "tn93":
            assert got[3].shape == (n_loaded, NW, k, 4) and got[3].dtype == np.uint32
        if measure in ("n", "raw"):      # the definition itself, without the GPU
            index, payloads = reference(measure, loaded, streamed, k)
            assert np.array_equal(got[0], index), (measure, n_loaded, k)
            ref = take(payloads, index)
            assert ((bits(got[1]) == bits(ref)) | (got[1] != got[1]) & (ref != ref)).all(), (measure, n_loaded, k)
    assert (got[0][:, 4, :3] == np.arange(3, dtype=np.uint32)).all()      # the empty window: the first ordinals


# ---- 2. the answer depends neither on the cut, nor on depth, nor on the wire ---------------------------------------------------
@pytest.mark.parametrize("nibbles", [False, True])
@pytest.mark.parametrize("depth", [2, 3])
def test_every_cut_gives_the_same_bits(eng, data, depth, nibbles):
    loaded, streamed = data
    eng.upload(0, loaded)
    for measure, k in (("n_high", 3), ("raw", 65), ("tn93", 3)):
        want = yardstick(eng, measure, 9, k, streamed)
        for cut in CUTS:
            got = run_stream(eng, measure, k, streamed, cut, depth=depth, nibbles=nibbles)
            assert_same(got, want, (measure, depth, nibbles, cut[:2]))


# ---- 3. ... nor on max_entries ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_entries", [1, 257 * 8, 0])      # 1: every range one (record, window) list
def test_every_range_cut_gives_the_same_bits(eng, data, max_entries):
    loaded, streamed = data
    eng.upload(0, loaded)
    for measure in ("raw", "tn93"):
        want = yardstick(eng, measure, 9, 3, streamed)
        got = run_stream(eng, measure, 3, streamed, [257, 43], max_entries=max_entries)
        assert_same(got, want, (measure, max_entries))


# ---- 4. fewer records than k; snapshots ---------------------------------------------------------------------------------------------
def test_fewer_records_than_k_and_snapshots(eng, data):
    loaded, streamed = data
    eng.upload(0, loaded)
    whole = yardstick(eng, "tn93", 9, 65, streamed)
    first64 = yardstick(eng, "tn93", 9, 65, streamed[:64], tag="first 64")
    first3 = yardstick(eng, "tn93", 9, 65, streamed[:3], tag="first 3")
    assert first3[0].shape == (9, NW, 3)
    with eng.window_closest_stream("tn93", WINDOWS, 65, MAX_RECORDS) as st:
        idx, vals = st.result()
        assert idx.shape == (9, NW, 0) and vals.shape == (9, NW, 0)
        st.push(streamed[:3])
        assert st.pop() == 3
        assert_same(st.result(tallies=True, counts=True), first3, "k_used = records")
        st.push(streamed[3:64])
        assert st.pop() == 61
        half = st.result(tallies=True, counts=True)
        assert_same(half, first64, "mid-stream")
        assert_same(st.result(tallies=True, counts=True), half, "a snapshot twice")
        assert_same(st.result(), half[:2], "without tallies and counts")
        st.push(streamed[64:129])
        st.push(streamed[129:])
        assert st.pop() == 65 and st.pop() == 171
        assert_same(st.result(tallies=True, counts=True), whole, "after the rest")


# ---- 5. other window calls on the same engine between two pushes -------------------------------------------------------------
def test_other_window_calls_in_between(eng, data):
    loaded, streamed = data
    other = np.array([(10, 20), (0, 300), (250, 290)], np.uint64)
    eng.upload(0, loaded)
    want = {m: yardstick(eng, m, 9, 3, streamed) for m in ("tn93", "k80")}
    eng.upload(1, streamed[:50])
    theirs = {m: (eng.run_windows(m, other, square=False), eng.nearest_windows(m, other, 2, square=False, tallies=True),
                  eng.nearest_windows(m, other, 2, square=True)) for m in ("tn93", "k80")}
    for m in ("tn93", "k80"):
        with eng.window_closest_stream(m, WINDOWS, 3, MAX_RECORDS) as st:
            at = 0
            for n in TIE_CUT:
                st.push(streamed[at:at + n])
                at += n
                assert bits(eng.run_windows(m, other, square=False)).tobytes() == bits(theirs[m][0]).tobytes()
                assert_same(eng.nearest_windows(m, other, 2, square=False, tallies=True), theirs[m][1], m)
                assert_same(eng.nearest_windows(m, other, 2, square=True), theirs[m][2], m)
                assert eng.window_base_counts(0, other).shape == (3, 9, 4)
                st.pop()
            assert_same(st.result(tallies=True, counts=m == "tn93"), want[m], m)


# ---- 6. a loaded set whose planes are deferred ------------------------------------------------------------------------------------
def test_deferred_planes_of_the_loaded_set():
    n, length = 1100, 3333
    rng = np.random.default_rng(31)
    codes = synth.alignment(synth.SEED ^ 31, n + 100, length)
    for r in rng.choice(n + 100, 60, replace=False):
        at = rng.choice(length, 20, replace=False)
        codes[r, at] = CODES[rng.integers(0, 17, len(at))]
    loaded, streamed = codes[:n], codes[n:]
    windows = np.array([(0, length), (100, 1100), (127, 129), (3332, 3333), (500, 500)], np.uint64)
    with da.Engine(0) as dense, da.Engine(0) as lazy:
        dense.set_path("dense")
        dense.upload(0, loaded)
        dense.upload(1, streamed)
        assert dense.planes_stored(0)
        lazy.set_prep_threshold(0)
        lazy.upload(0, loaded)
        assert not lazy.planes_stored(0), "the upload stored every plane: nothing here tests the deferred form"
        for m in ("raw", "tn93"):
            want = dense.nearest_windows(m, windows, 4, square=False, tallies=True)
            got = run_stream(lazy, m, 4, streamed, [64, 36], max_records=64, windows=windows)
            assert lazy.planes_stored(0)
            assert_same(got[:3], want, m)


# ---- 7. ordinals ------------------------------------------------------------------------------------------------------------------------
def test_ordinals_compare_unsigned_across_2_31(eng, data):
    loaded, streamed = data[0], data[1][:12].copy()
    streamed[:] = streamed[0]                                  # twelve copies: every key ties, the ordinal decides
    eng.upload(0, loaded)
    first = 2**31 - 3
    got = run_stream(eng, "raw", 8, streamed, [4, 4, 4], max_records=4, first_index=first)
    want = yardstick(eng, "raw", 9, 8, streamed, tag="twelve copies")
    assert (want[0] == np.arange(8, dtype=np.uint32)).all()
    assert np.array_equal(got[0], want[0] + np.uint32(first)) and got[0].dtype == np.uint32
    assert got[0][0, 0].tolist() == [first + i for i in range(8)]    # 2^31 - 3 .. 2^31 + 4, ascending as unsigned
    assert_same(got[1:], want[1:])


def test_ordinals_end_at_2_32_minus_2(eng, data):
    loaded, streamed = data
    eng.upload(0, loaded)
    want = yardstick(eng, "raw", 9, 5, streamed[:64], tag="first 64")
    first = 2**32 - 70
    with eng.window_closest_stream("raw", WINDOWS, 5, 64) as st:
        st.next_index(first)
        st.push(streamed[:64])
        assert st.pop() == 64
        before = st.result(tallies=True)
        assert np.array_equal(before[0], want[0] + np.uint32(first)) and int(before[0].max()) <= 2**32 - 7
        assert_same(before[1:], want[1:])
        assert status_of(st.push, streamed[64:74]) == ERR_CAPACITY        # 2^32 - 6 + 9 passes 2^32 - 2
        assert st.in_flight() == 0
        assert_same(st.result(tallies=True), before)
        st.submit(4)                   # (the refused buffer is still acquired) 2^32 - 6 .. 2^32 - 3 still fit
        assert st.pop() == 4
        assert int(st.result()[0].max()) <= 2**32 - 3


def test_next_index_misuse(eng, data):
    loaded, streamed = data
    eng.upload(0, loaded)
    with eng.window_closest_stream("raw", WINDOWS, 5, 64) as st:
        st.next_index(100)
        assert status_of(st.next_index, 99) == ERR_ARG                   # backwards
        assert status_of(st.next_index, 2**32) == ERR_ARG
        st.push(streamed[:10])
        assert status_of(st.next_index, 1000) == ERR_STATE               # a batch in flight
        st.pop()
        assert status_of(st.next_index, 109) == ERR_ARG                  # ten records went by
        st.next_index(110)
        idx, _ = st.result()
        assert idx.min() >= 100 and idx.max() <= 109 and idx.shape == (9, NW, 5)


# ---- 8. the documented statuses ----------------------------------------------------------------------------------------------------
def test_open_errors(eng, data):
    lib = da.load()
    loaded, streamed = data
    eng.upload(0, loaded)
    wb, we = np.ascontiguousarray(WINDOWS[:, 0]), np.ascontiguousarray(WINDOWS[:, 1])
    h = C.c_void_p()

    def open_raw(ctx=None, measure=2, k=3, b=wb.ctypes.data, e=we.ctypes.data, nw=NW, max_records=8, depth=3, wire=0, out=C.byref(h)):
        return lib.dst_stream_open_window_closest(eng._h if ctx is None else ctx, measure, k, b, e, nw, 0, max_records, depth, wire, out)

    assert lib.dst_stream_open_window_closest(None, 2, 3, wb.ctypes.data, we.ctypes.data, NW, 0, 8, 3, 0, C.byref(h)) == ERR_ARG
    assert open_raw(out=None) == ERR_ARG
    assert open_raw(measure=6) == ERR_ARG and open_raw(measure=-1) == ERR_ARG and open_raw(wire=2) == ERR_ARG
    assert open_raw(k=0) == ERR_ARG and open_raw(k=257) == ERR_ARG
    assert open_raw(nw=0) == ERR_ARG and open_raw(nw=da.WINDOWS_MAX + 1) == ERR_ARG
    assert open_raw(b=None) == ERR_ARG and open_raw(e=None) == ERR_ARG
    assert open_raw(max_records=0) == ERR_ARG and open_raw(depth=1) == ERR_ARG and open_raw(depth=17) == ERR_ARG
    assert h.value is None
    with da.Engine(0) as fresh:
        assert open_raw(ctx=fresh._h) == ERR_STATE             # slot 0 not loaded
        assert open_raw(ctx=fresh._h, k=0) == ERR_ARG          # ... comes after the arguments
        assert h.value is None
    for bad, name in ((np.array([(0, 300), (5, 4)], np.uint64), "window 1"), (np.array([(0, 301)], np.uint64), "window 0")):
        with pytest.raises(da.DistanceError) as e:
            eng.window_closest_stream("raw", bad, 3, 8)
        assert e.value.status == ERR_ARG and name in e.value.message
    # n_loaded x n_windows lists above what the kernel indexes (2^31): the argument check, nothing is allocated
    many = np.zeros((da.WINDOWS_MAX, 2), np.uint64)
    with da.Engine(0) as big:
        big.upload(0, np.full((2**15 + 1, 1), 136, np.uint8))
        with pytest.raises(da.DistanceError) as e:
            big.window_closest_stream("n", many, 1, 8)
        assert e.value.status == ERR_ARG and "2^31" in e.value.message
    # what does not fit: DST_ERR_NOMEM with the byte count
    with pytest.raises(da.DistanceError) as e:
        eng.window_closest_stream("tn93", WINDOWS, 3, 2**40)
    assert e.value.status == ERR_NOMEM and "bytes" in e.value.message and any(c.isdigit() for c in e.value.message)
    # submit: the loaded set changed
    with eng.window_closest_stream("raw", WINDOWS, 3, 8) as st:
        eng.upload(0, loaded[:5])
        assert status_of(st.push, streamed[:8]) == ERR_STATE
        eng.upload(0, np.ascontiguousarray(loaded[:, :200]))
        assert status_of(st.submit, 8) == ERR_STATE
    eng.upload(0, loaded)


def test_shared_set_is_refused():
    """Slot 0 from dst_upload_shared: DST_ERR_STATE with the dense kernels' refusal, and no stream handle.
    Two open errors of the list cannot be reached by a test: an alignment of 2^32 sites or more and a loaded set of 2^32-1
    records or more cannot be allocated (dst_upload would have to hold them), so those two checks are read, not run."""
    from shared_ranks import ThreadRanks
    from test_gpu_window_nearest import Hip
    n, length = 2_500, 3_000   # (a shape of test_gpu_shared: the lists fit their blocks, no rank falls back to a full upload)
    codes = synth.alignment(synth.SEED ^ 9, n, length)
    hip = Hip()
    d_codes = hip.to_device(codes)
    windows = np.array([(0, 100), (50, 3_000)], np.uint64)
    wb, we = np.ascontiguousarray(windows[:, 0]), np.ascontiguousarray(windows[:, 1])
    lib = da.load()

    def body(rank, eng, comm):
        eng.upload_shared(comm, 0, d_codes, n, length, length, with_counts=True)
        assert eng.shared_stats()["fallbacks"] == 0
        out = []
        for measure in (2, 5):      # raw, tn93
            h = C.c_void_p()
            rc = lib.dst_stream_open_window_closest(eng._h, measure, 3, wb.ctypes.data, we.ctypes.data, 2, 0, 8, 3, 0, C.byref(h))
            out.append((rc, lib.dst_last_error(eng._h).decode(), h.value))
        with pytest.raises(da.DistanceError) as e:
            eng.window_closest_stream("raw", windows, 3, 8)
        return out + [(e.value.status, e.value.message, None)]

    try:
        for results in ThreadRanks(2).run(body):
            for status, message, handle in results:
                assert status == ERR_STATE and "dst_upload_shared runs on the consensus path only" in message
                assert handle is None
    finally:
        hip.lib.hipFree(d_codes)


def test_result_errors_and_the_other_streams_calls(eng, data):
    lib = da.load()
    loaded, streamed = data
    eng.upload(0, loaded)
    ip, tp, vp, ku = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint32(7)
    n64, t64 = C.c_uint64(), C.c_uint64()
    index = np.zeros(9 * NW * 5, np.uint32)
    with eng.window_closest_stream("raw", WINDOWS, 5, 8) as st:
        assert status_of(st.result, counts=True) == ERR_ARG                      # counts are tn93's
        st.push(streamed[:8])
        assert status_of(st.result) == ERR_STATE                                 # a batch in flight
        n, p = C.c_size_t(), C.c_void_p(1)
        assert lib.dst_stream_collect(st._h, C.byref(n), C.byref(p)) == 0 and n.value == 8 and p.value is None
        assert lib.dst_stream_window_closest_result(st._h, index.ctypes.data, None, None, None, 9 * NW * 5 - 1, C.byref(ku)) == ERR_CAPACITY
        assert ku.value == 5                                                     # ... with *k_used set
        assert lib.dst_stream_window_closest_result(st._h, None, None, None, None, index.size, C.byref(ku)) == ERR_ARG
        assert lib.dst_stream_window_closest_result(st._h, index.ctypes.data, None, None, None, index.size, None) == ERR_ARG
        assert st.result()[0].shape == (9, NW, 5)
        # the other closest and links calls on it
        assert lib.dst_stream_closest_result(st._h, index.ctypes.data, None, None, index.size, C.byref(ku)) == ERR_ARG
        assert lib.dst_stream_closest_batch(st._h, C.byref(ip), C.byref(tp), C.byref(vp), C.byref(ku)) == ERR_ARG
        assert lib.dst_stream_links_batch(st._h, 0, C.byref(n64), C.byref(t64), C.byref(ip), C.byref(tp), None, None) == ERR_ARG
        assert lib.dst_stream_links_stats(st._h, C.byref(n64), C.byref(t64)) == ERR_ARG
    # this one's call on the other streams
    for other in (eng.stream("raw", max_records=8, depth=2), eng.closest_stream("raw", 5, 8), eng.closest_stream("raw", 5, 8, side="streamed"),
                  eng.links_stream("raw", 0.1, 8)):
        with other as st:
            assert lib.dst_stream_window_closest_result(st._h, index.ctypes.data, None, None, None, index.size, C.byref(ku)) == ERR_ARG
    assert lib.dst_stream_window_closest_result(None, index.ctypes.data, None, None, None, index.size, C.byref(ku)) == ERR_ARG


@pytest.mark.parametrize("nibbles", [False, True])
def test_an_invalid_code_poisons_the_lists(eng, data, nibbles):
    loaded, streamed = data
    eng.upload(0, loaded)
    with eng.window_closest_stream("raw", WINDOWS, 5, 8, nibbles=nibbles) as st:
        st.push(streamed[:8])
        buf, _ = st.buffer()
        if nibbles:
            nib = da.engine.Stream.to_nibbles(streamed[8:12])
            nib[2, 100] &= 0x0F                                  # site 201 of record 2: nibble 0
            buf[:4] = nib
        else:
            bad = streamed[8:12].copy()
            bad[2, 200] = 7
            buf[:4] = bad
        st.submit(4)
        assert st.pop() == 8
        with pytest.raises(da.DistanceError) as e:
            st.pop()
        assert e.value.status == ERR_INVALID_CODE and "record 2 at site 20" in e.value.message
        assert status_of(st.result) == ERR_STATE
        assert status_of(st.push, streamed[:4]) == ERR_STATE
