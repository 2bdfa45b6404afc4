"""GPU (-m gpu): summary streams (dst_stream_open_summary / Engine.summary_stream) - dst_summary's counts and exact sums kept
instead of a batch's result matrix - against the plain stream's own matrix S[streamed][loaded] of the same records reduced by
the numpy restatement of the definition (summary_reference): S for the streamed side, the histogram and the totals, S.T
for the loaded side.  Integers are compared for equality and sums bitwise; there is no tolerance anywhere.  Every measure
across the tile's column and row boundaries, the thresholds, the sides, the histogram, every cut of the stream, NaN / +inf
/ duplicates / both sum words, tn93's counts, the kernel paths, snapshots with other calls in between, ring reuse, an
invalid code and the documented errors."""
import ctypes as C

import numpy as np
import pytest

import distance_amd as da
import oracle
from closest_reference import bits, cuts_of, plain_truth, special_values_set
from helpers import alignment_root, random_alignment
from summary_reference import assert_summary, summary
from tools import synth

pytestmark = pytest.mark.gpu
ALL = ("n", "n_high", "raw", "jc69", "k80", "tn93")
ERR_ARG, ERR_INVALID_CODE, ERR_STATE, ERR_CAPACITY = 1, 3, 4, 6
R, COLS = da._lib.STREAM_SUMMARY_ROWS, da._lib.STREAM_SUMMARY_COLS
L, N_S, MAXREC = 96, 70, 32
INF = float("inf")
WHATS = [(False, False), (True, False), (False, True), (True, True)]   # (loaded, streamed)


@pytest.fixture(scope="module")
def eng():
    e = da.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def data():
    """2,049 loaded and 70 streamed records of one alignment; every 41st record is far from the rest (the root's
    complement), so n reaches the 64th bin of width 1 and jc69 / k80 saturate"""
    both = random_alignment(2049 + N_S, L, seed=401)
    root = alignment_root(L, 401)
    alt = np.array([{136: 72, 72: 136, 40: 24, 24: 40}[int(c)] for c in root], np.uint8)
    far = random_alignment(64, L, seed=402, root=alt)
    both[5::41] = far[:len(both[5::41])]
    return both[:2049], both[2049:]


_truth = {}


def truth(eng, tag, measure, streamed, counts=None):
    """the plain stream's S of the set uploaded to slot 0, computed once per (set, measure, flag) and never changed"""
    key = (tag, measure, counts is not None)
    if key not in _truth:
        _truth[key] = plain_truth(eng, measure, streamed, counts, max_records=MAXREC)[0]
    return _truth[key]


def reference(measure, S, T, bins=0, width=1.0):
    """(what result() must return with both sides and the histogram, what the streamed side must be) from S"""
    n_s, n_l = S.shape
    rows = summary(measure, S, n_s, n_l, False, T, bins, width)
    cols = summary(measure, np.ascontiguousarray(S.T), n_l, n_s, False, T)
    for key in ("pairs", "nan_pairs", "summable_pairs", "links"):
        assert rows[key] == cols[key]
    want = dict(rows, records=n_s, within=cols["within"], summable=cols["summable"], sum=cols["sum"])
    return want, (rows["within"], rows["summable"], rows["sum"])


def run_summary(eng, measure, T, streamed, cuts, loaded=True, streamed_side=False, bins=0, width=1.0, counts=None,
                max_records=MAXREC, depth=3, nibbles=False):
    """Push `streamed` cut into batches of the sizes `cuts` through a summary stream, popping as the ring fills: result()
    and the batches' streamed side concatenated (None without it)."""
    got, b0 = [], 0
    with eng.summary_stream(measure, max_records, threshold=T, loaded=loaded, streamed=streamed_side, bins=bins, width=width,
                            depth=depth, nibbles=nibbles) as st:
        for size in cuts:
            if st.in_flight() == depth - 1:
                got.append(st.pop())
            st.push(streamed[b0:b0 + size], None if counts is None else counts[b0:b0 + size])
            b0 += size
        assert b0 == len(streamed)
        while st.in_flight():
            got.append(st.pop())
        res = st.result()
    if not streamed_side:
        assert got == list(cuts)
        return res, None
    assert [g[0] for g in got] == list(cuts)
    return res, tuple(np.concatenate([g[a] for g in got]) for a in (1, 2, 3))


def check(got, want, what=""):
    """result() against the reference: the keys a stream opened like this one must and must not return, then the bits"""
    res, side = got
    want_res, want_side = want
    assert res["records"] == want_res["records"], what
    assert ("within" in res) == ("summable" in res) == ("sum" in res), what
    assert_summary(res, want_res, what)
    if side is not None:
        assert side[0].dtype == np.uint32 and side[1].dtype == np.uint32 and side[2].dtype == np.float64, what
        assert np.array_equal(side[0], want_side[0]), (what, "streamed within")
        assert np.array_equal(side[1], want_side[1]), (what, "streamed summable")
        assert np.array_equal(bits(side[2]), bits(want_side[2])), (what, "streamed sum")


def status_of(fn, *a, **kw):
    with pytest.raises(da.DistanceError) as e:
        fn(*a, **kw)
    return e.value.status


def median_of(S):
    flat = S.reshape(-1)
    return float(np.median(flat[np.isfinite(flat)] if flat.dtype == np.float64 else flat))


def last_bin_width(measure, S):
    """a width that leaves the upper half of the finite values to the last of 64 bins"""
    flat = S.reshape(-1).astype(np.float64)
    top = float(flat[np.isfinite(flat)].max())
    return float(max(1, int(top) // 128)) if measure in da.INT_MEASURES else top / 128


# ---- 1. every measure across the tile's column boundary, the thresholds, the sides, the histogram --------------------------
@pytest.mark.parametrize("measure", ALL)
@pytest.mark.parametrize("n_loaded", [1, COLS - 1, COLS, COLS + 1, 2049])
def test_every_measure_threshold_and_side_against_the_plain_stream(eng, data, n_loaded, measure):
    loaded, streamed = data[0][:n_loaded], data[1]
    eng.upload(0, loaded)
    S = truth(eng, n_loaded, measure, streamed)
    assert S.shape == (N_S, n_loaded)
    if measure in ("n", "n_high", "raw") and n_loaded <= COLS:     # the truth itself is pinned
        want = oracle.all_pairs_rect(measure, streamed, loaded)
        want = want.astype(np.int64) if measure in da.INT_MEASURES else want
        assert np.array_equal(bits(S), bits(want)), measure
    cuts = cuts_of(N_S, MAXREC)
    med = median_of(S)
    for T in (-1.0, med, INF):
        want = reference(measure, S, T)
        for lo, st in WHATS:
            got = run_summary(eng, measure, T, streamed, cuts, loaded=lo, streamed_side=st)
            assert ("within" in got[0]) == lo and (got[1] is not None) == st and "hist" not in got[0]
            check(got, want, (measure, n_loaded, T, lo, st))
        assert want[0]["pairs"] == N_S * n_loaded
        if T == -1.0:
            assert want[0]["links"] == 0
        if T == INF:
            assert want[0]["links"] == want[0]["pairs"] - want[0]["nan_pairs"]
    if n_loaded > 1:
        assert 0 < reference(measure, S, med)[0]["links"] < S.size
    wide = last_bin_width(measure, S)
    for bins, width in ((1, wide), (64, wide)):
        want = reference(measure, S, med, bins, width)
        assert int(want[0]["hist"][-1]) > 0, (measure, bins, width)            # values in the last, open bin
        if bins > 1 and n_loaded > 1:
            assert int(want[0]["hist"][:-1].sum()) > 0
        for lo, st in WHATS:
            got = run_summary(eng, measure, med, streamed, cuts, loaded=lo, streamed_side=st, bins=bins, width=width)
            assert got[0]["hist"].shape == (bins,)
            check(got, want, (measure, n_loaded, bins, lo, st))


# ---- 2. the tile's rows -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", ["n", "k80", "tn93"])
def test_tile_rows_and_the_rectangle_form(eng, measure):
    sizes = [1, R - 1, R, R + 1, 2 * R + 1]
    both = random_alignment(COLS + 1 + sum(sizes), L, seed=411)
    loaded, streamed = both[:COLS + 1], both[COLS + 1:]
    eng.upload(0, loaded)
    S = plain_truth(eng, measure, streamed, max_records=2 * R + 1)[0]
    T = median_of(S)
    got = run_summary(eng, measure, T, streamed, sizes, streamed_side=True, bins=16, width=last_bin_width(measure, S),
                      max_records=2 * R + 1)
    check(got, reference(measure, S, T, 16, last_bin_width(measure, S)), measure)
    # the streamed side of each batch is dst_summary's rectangle with the batch as rows
    with da.Engine(0) as other:
        other.upload(0, loaded)
        b0 = 0
        for size in sizes:
            other.upload(1, streamed[b0:b0 + size])
            rect = other.summary(measure, threshold=T, square=False, row_slot=1, col_slot=0)
            for a, key in enumerate(("within", "summable", "sum")):
                assert np.array_equal(bits(got[1][a][b0:b0 + size]), bits(rect[key])), (measure, size, key)
            b0 += size


# ---- 3. the answer does not depend on the cut ----------------------------------------------------------------------------------
@pytest.mark.parametrize("nibbles", [False, True])
@pytest.mark.parametrize("depth", [2, 3])
def test_every_cut_gives_the_same_bits(eng, data, depth, nibbles):
    loaded, streamed = data[0][:COLS + 1], data[1]
    eng.upload(0, loaded)
    for measure in ("n_high", "k80"):
        S = truth(eng, COLS + 1, measure, streamed)
        T = median_of(S)
        width = last_bin_width(measure, S)
        want = reference(measure, S, T, 64, width)
        results = []
        for cut in ([N_S], cuts_of(N_S, 1), [32, 5, 1, 32]):
            got = run_summary(eng, measure, T, streamed, cut, streamed_side=True, bins=64, width=width, max_records=N_S,
                              depth=depth, nibbles=nibbles)
            check(got, want, (measure, depth, nibbles, cut[0]))
            results.append(got)
        for other in results[1:]:
            for key in ("within", "summable", "sum", "hist"):
                assert np.array_equal(bits(other[0][key]), bits(results[0][0][key])), key
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(other[1], results[0][1]))


# ---- 4. special values -------------------------------------------------------------------------------------------------------
def test_special_values(eng):
    base = special_values_set()
    loaded = base[[0, 12, 22, 30, 31, 32, 1]]              # a root, a saturated one, all N, three ordinary, the root again
    streamed = base
    eng.upload(0, loaded)
    for m in ALL:
        S = plain_truth(eng, m, streamed, max_records=16)[0]
        res = {}
        for T in (0.0, 0.5, 1e300, INF):
            want = reference(m, S, T, 8, 1.0 if m in da.INT_MEASURES else 0.125)
            res[T] = run_summary(eng, m, T, streamed, cuts_of(40, 16), streamed_side=True, bins=8,
                                 width=1.0 if m in da.INT_MEASURES else 0.125, max_records=16)
            check(res[T], want, (m, T))
        at_0, at_inf = res[0.0][0], res[INF][0]
        assert at_0["within"][0] >= 10 and at_0["within"][6] == at_0["within"][0]      # duplicates link at T = 0
        if m in da.INT_MEASURES:
            continue
        # raw NaN: an all-N record on either side is summable with nobody, links with nobody and lies in no bin
        assert at_inf["nan_pairs"] == int(np.isnan(S).sum()) >= 40 + 5 * 6
        assert at_inf["summable"][2] == 0 and at_inf["within"][2] == 0 and at_inf["sum"][2] == 0.0
        assert (res[INF][1][1][20:25] == 0).all() and (res[INF][1][0][20:25] == 0).all()
        assert int(at_inf["hist"].sum()) == at_inf["pairs"] - at_inf["nan_pairs"]
        if m == "jc69":                                    # +inf links only at T = inf, lies in the last bin, is not summable
            n_inf = int(np.isposinf(S).sum())
            assert n_inf >= 10
            assert at_inf["links"] - res[1e300][0]["links"] == n_inf
            assert at_inf["summable_pairs"] == at_inf["pairs"] - at_inf["nan_pairs"] - n_inf
            assert int(at_inf["hist"][-1]) >= n_inf
        if m == "raw":                                     # 0.75 2^37 is above 2^32: both words of the sums are in use
            assert S[np.isfinite(S)].max() >= 0.7 and at_inf["sum"].max() > 5.0


# ---- 5. tn93's counts ----------------------------------------------------------------------------------------------------------
def test_tn93_with_device_counts_and_with_the_callers(eng, data):
    loaded, streamed = data[0][:COLS + 1], data[1]
    eng.upload(0, loaded)
    counts = oracle.count_bases_matrix(streamed).astype(np.uint32)
    counts[:, 0] += (np.arange(N_S) % 3).astype(np.uint32) * 5      # the caller's counts are the caller's: not the device's
    S0 = truth(eng, COLS + 1, "tn93", streamed)
    S1 = truth(eng, COLS + 1, "tn93", streamed, counts)
    assert not np.array_equal(bits(S0), bits(S1))
    T = median_of(S0)
    cuts = cuts_of(N_S, MAXREC)
    got0 = run_summary(eng, "tn93", T, streamed, cuts, streamed_side=True, bins=32, width=0.01)
    got1 = run_summary(eng, "tn93", T, streamed, cuts, streamed_side=True, bins=32, width=0.01, counts=counts)
    check(got0, reference("tn93", S0, T, 32, 0.01), "device counts")
    check(got1, reference("tn93", S1, T, 32, 0.01), "caller's counts")
    assert not np.array_equal(bits(got0[0]["sum"]), bits(got1[0]["sum"]))


# ---- 6. kernel paths -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["low", "random"])
def test_kernel_paths_give_the_same_bits(kind):
    if kind == "low":
        r = synth.root(synth.SEED, 3000)
        both = synth.records(synth.SEED, r, 0, 130 + 100)
    else:
        both = random_alignment(130 + 100, 3000, seed=311)
    loaded, streamed = both[:130], both[130:]
    with da.Engine(0) as e:
        e.set_prep_threshold(0)
        e.upload(0, loaded)
        e.set_path("dense")
        truths = {m: plain_truth(e, m, streamed, max_records=64)[0] for m in ("raw", "tn93")}
        T = {m: median_of(truths[m]) for m in truths}
        for path in ("dense", "consensus", "auto"):
            e.set_path(path)
            for m in ("raw", "tn93"):
                got = run_summary(e, m, T[m], streamed, cuts_of(100, 64), streamed_side=True, bins=16, width=0.001, max_records=64)
                if kind == "low" and path != "auto":      # (a low-diversity set is what the lists index: no fall-back)
                    assert e.last_path() == path, (path, m)
                check(got, reference(m, truths[m], T[m], 16, 0.001), (kind, path, m))


# ---- 7. snapshots, and other calls on the context in between -------------------------------------------------------------------
def test_snapshots_and_other_calls_in_between(data):
    loaded, streamed = data[0][:COLS + 1], data[1]
    with da.Engine(0) as e:
        e.upload(0, loaded)
        S = plain_truth(e, "k80", streamed, max_records=MAXREC)[0]
        Sn = plain_truth(e, "n", streamed, max_records=MAXREC)[0]
        T = median_of(S)
        square_before = e.summary("k80", threshold=T, bins=8, width=0.05)
        with e.summary_stream("k80", 16, threshold=T, streamed=True, bins=8, width=0.05) as st, \
                e.summary_stream("n", 16, threshold=3, depth=2) as second:
            assert st.result()["records"] == 0 and st.result()["pairs"] == 0 and not st.result()["within"].any()
            for b0 in range(0, 64, 16):
                st.push(streamed[b0:b0 + 16])
                # the context's own summary (ctx->summary_work), links and nearest between a submit and its collect
                assert_summary(e.summary("k80", threshold=T, bins=8, width=0.05), square_before, "dst_summary in between")
                e.links("k80", T)
                e.nearest("k80", 3)
                second.push(streamed[b0:b0 + 16])
                side = st.pop()
                assert second.pop() == 16
                want = reference("k80", S[:b0 + 16], T, 8, 0.05)
                check((st.result(), None), want, ("snapshot", b0))
                check((st.result(), None), want, ("snapshot again", b0))
                assert all(np.array_equal(bits(a), bits(b[b0:b0 + 16])) for a, b in zip(side[1:], want[1])), b0
                check((second.result(), None), reference("n", Sn[:b0 + 16], 3), ("second stream", b0))
        assert_summary(e.summary("k80", threshold=T, bins=8, width=0.05), square_before, "dst_summary afterwards")


# ---- 8. ring reuse ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [2, 3])
def test_ring_reuse_popping_late(eng, data, depth):
    loaded, streamed = data[0][:COLS + 1], data[1]
    eng.upload(0, loaded)
    S = truth(eng, COLS + 1, "raw", streamed)
    T = median_of(S)
    want = reference("raw", S[:64], T)
    popped = 0
    with eng.summary_stream("raw", 8, threshold=T, streamed=True, depth=depth) as st:
        for b0 in range(0, 64, 8):                               # eight batches through two or three slots
            if st.in_flight() == depth:                          # every slot is in flight: the oldest batch, as late as can be
                first = st.pop()
                again = st.summary_batch()                       # valid from collect to the next submit
                assert first[0] == again[0] == 8
                for a in (1, 2, 3):
                    assert np.array_equal(bits(first[a]), bits(again[a]))
                    assert np.array_equal(bits(first[a]), bits(want[1][a - 1][popped:popped + 8])), (b0, a)
                popped += 8
            st.push(streamed[b0:b0 + 8])
            assert status_of(st.summary_batch) == ERR_STATE      # the submit ended the collected batch's validity
        while st.in_flight():
            got = st.pop()
            for a in (1, 2, 3):
                assert np.array_equal(bits(got[a]), bits(want[1][a - 1][popped:popped + 8])), (popped, a)
            popped += 8
        assert popped == 64
        check((st.result(), None), want, depth)


# ---- 9. an invalid code ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nibbles", [False, True])
def test_an_invalid_code_poisons_the_stream(eng, data, nibbles):
    loaded, streamed = data[0][:COLS + 1], data[1]
    eng.upload(0, loaded)
    S = truth(eng, COLS + 1, "raw", streamed)
    with eng.summary_stream("raw", 8, threshold=0.05, streamed=True, nibbles=nibbles) as st:
        st.push(streamed[:8])
        buf, _ = st.buffer()
        if nibbles:
            nib = da.engine.Stream.to_nibbles(streamed[8:12])
            nib[2, 30] &= 0x0F                                   # site 61 of record 2: nibble 0
            buf[:4] = nib
        else:
            bad = streamed[8:12].copy()
            bad[2, 60] = 7
            buf[:4] = bad
        st.submit(4)
        assert st.pop()[0] == 8
        with pytest.raises(da.DistanceError) as e:
            st.pop()
        assert e.value.status == ERR_INVALID_CODE and "record 2 at site 6" in e.value.message
        assert status_of(st.summary_batch) == ERR_STATE
        assert status_of(st.result) == ERR_STATE
        assert status_of(st.push, streamed[12:20]) == ERR_STATE  # the batch's atomics cannot be taken back
        assert status_of(st.result) == ERR_STATE
    # close worked; a fresh stream on the same context gives the right answer
    check(run_summary(eng, "raw", 0.05, streamed, cuts_of(N_S, MAXREC), streamed_side=True), reference("raw", S, 0.05), "fresh")


# ---- 10. misuse: the documented statuses -------------------------------------------------------------------------------------------
def test_open_errors_in_the_documented_order(eng, data):
    lib = da.load()
    eng.upload(0, data[0][:130])
    h = C.c_void_p()

    def open_(ctx, measure=2, T=1.0, what=3, bins=0, width=1.0, max_records=8, depth=3, wire=0, out=C.byref(h)):
        return lib.dst_stream_open_summary(ctx, measure, T, what, bins, width, max_records, depth, wire, out)

    assert open_(None) == ERR_ARG and open_(eng._h, out=None) == ERR_ARG
    for bad in (dict(measure=9), dict(measure=-1), dict(wire=2), dict(T=float("nan")), dict(what=4), dict(what=-1),
                dict(bins=4097), dict(bins=4, width=0.0), dict(bins=4, width=-1.0), dict(bins=4, width=float("nan")),
                dict(bins=4, width=float("inf")), dict(bins=4, width=2.0 ** 25), dict(bins=4, width=2.0 ** -39),
                dict(bins=4, width=1.5, measure=0), dict(max_records=0), dict(depth=1), dict(depth=17)):
        assert open_(eng._h, **bad) == ERR_ARG, bad
        assert h.value is None
    for message, bad in (("bins must be between 0 and 4096", dict(bins=4097)),
                         ("width must be finite, above 0 and below 2^25", dict(bins=4, width=0.0)),
                         ("width must be an integer for n and n_high", dict(bins=4, width=1.5, measure=1)),
                         ("width is below one unit of the fixed-point scale", dict(bins=4, width=2.0 ** -39)),
                         ("threshold is NaN", dict(T=float("nan")))):
        assert open_(eng._h, **bad) == ERR_ARG and message in lib.dst_last_error(eng._h).decode(), message
    assert open_(eng._h, bins=0, width=float("nan")) == 0                 # bins == 0: the width is ignored, as dst_summary's
    lib.dst_stream_close(h)
    with da.Engine(0) as fresh:                                            # slot 0 not loaded: behind every argument error
        assert status_of(fresh.summary_stream, "raw", 8) == ERR_STATE
        assert open_(fresh._h, what=4) == ERR_ARG and open_(fresh._h, depth=1) == ERR_ARG and open_(fresh._h, bins=4097) == ERR_ARG


def test_misuse(eng, data):
    lib = da.load()
    loaded, streamed = data[0][:130], data[1]
    eng.upload(0, loaded)
    n, wp, sp, dp, ku = C.c_size_t(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint32()
    total, late = C.c_uint64(), C.c_uint64()
    every = (C.byref(n), C.byref(wp), C.byref(sp), C.byref(dp))
    room = np.zeros(130, np.uint32)
    sums = np.zeros(130, np.float64)
    hist = np.zeros(8, np.uint64)

    def result(st, hist=None, within=None, summable=None, sum_=None, cap=130):
        return lib.dst_stream_summary_result(st._h, hist, within, summable, sum_, cap, None, None)

    with eng.summary_stream("raw", 8, threshold=0.05, streamed=True, bins=8, width=0.01) as st:
        assert lib.dst_stream_summary_batch(st._h, *every) == ERR_STATE              # no collected batch
        st.push(streamed[:8])
        assert lib.dst_stream_summary_batch(st._h, *every) == ERR_STATE
        assert status_of(st.result) == ERR_STATE                                     # a batch in flight
        assert st.pop()[0] == 8
        assert lib.dst_stream_summary_batch(st._h, None, *every[1:]) == ERR_ARG
        assert lib.dst_stream_summary_batch(st._h, C.byref(n), None, None, None) == 0 and n.value == 8
        assert result(st, within=room.ctypes.data, cap=129) == ERR_CAPACITY          # cap below n_loaded
        assert result(st, sum_=sums.ctypes.data, cap=0) == ERR_CAPACITY
        assert result(st, hist=hist.ctypes.data, cap=0) == 0 and int(hist.sum()) > 0 # no per-record array: cap is not read
        assert result(st, within=room.ctypes.data, summable=room.ctypes.data, sum_=sums.ctypes.data) == 0
        # the other kinds' calls on this stream
        index = np.zeros(1040, np.uint32)
        assert lib.dst_stream_closest_batch(st._h, C.byref(sp), C.byref(wp), C.byref(dp), C.byref(ku)) == ERR_ARG
        assert lib.dst_stream_closest_result(st._h, index.ctypes.data, None, None, 1040, C.byref(ku)) == ERR_ARG
        assert lib.dst_stream_closest_next_index(st._h, 5) == ERR_ARG
        assert lib.dst_stream_links_batch(st._h, 0, C.byref(total), C.byref(late), C.byref(sp), C.byref(wp), None, None) == ERR_ARG
        assert lib.dst_stream_links_stats(st._h, C.byref(total), C.byref(late)) == ERR_ARG
        assert lib.dst_stream_window_closest_result(st._h, index.ctypes.data, None, None, None, 1040, C.byref(ku)) == ERR_ARG
        eng.upload(0, loaded[:100])                                                  # the loaded set's record count changed
        assert status_of(st.push, streamed[:8]) == ERR_STATE
    eng.upload(0, loaded)
    with eng.summary_stream("raw", 8, threshold=0.05, loaded=False, streamed=True) as st:     # a side that was not asked for
        st.push(streamed[:8])
        st.pop()
        for kw in (dict(within=room.ctypes.data), dict(summable=room.ctypes.data), dict(sum_=sums.ctypes.data)):
            assert result(st, **kw) == ERR_ARG, kw
        assert result(st) == 0
    with eng.summary_stream("raw", 8, threshold=0.05) as st:                         # ... and the other one
        st.push(streamed[:8])
        assert st.pop() == 8
        assert lib.dst_stream_summary_batch(st._h, *every) == ERR_ARG
    # this kind's calls on the other kinds, and on no stream at all
    for other in (eng.stream("raw", max_records=8, depth=2), eng.closest_stream("raw", 5, 8),
                  eng.closest_stream("raw", 5, 8, side="streamed"), eng.links_stream("raw", 0.05, 8),
                  eng.window_closest_stream("raw", [(0, 48), (48, 96)], 2, 8)):
        with other as st:
            assert lib.dst_stream_summary_batch(st._h, *every) == ERR_ARG
            assert result(st) == ERR_ARG
    assert lib.dst_stream_summary_batch(None, *every) == ERR_ARG
    assert lib.dst_stream_summary_result(None, None, None, None, None, 0, None, None) == ERR_ARG


def test_a_plain_stream_afterwards(data):
    """(An empty loaded set cannot arise: dst_upload refuses n = 0.)"""
    loaded, streamed = data[0][:130], data[1]
    with da.Engine(0) as e:
        e.upload(0, loaded)
        before = plain_truth(e, "tn93", streamed, max_records=MAXREC)
        S = before[0]
        check(run_summary(e, "tn93", 0.05, streamed, cuts_of(N_S, MAXREC), streamed_side=True, bins=4, width=0.02),
              reference("tn93", S, 0.05, 4, 0.02), "tn93")
        after = plain_truth(e, "tn93", streamed, max_records=MAXREC)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(after, before))   # a plain stream still delivers its matrix
