"""GPU (-m gpu): links streams (dst_stream_open_links / Engine.links_stream) — the pairs within a threshold handed back
instead of a batch's result matrix — against the plain stream's own results of the same batches filtered by the documented
rule (links_reference.linked), bit for bit: every measure across the 2,048-entry block boundary of a row, the thresholds,
the windows, every cut of the stream, NaN / +inf / -0.0, tn93's counts, the kernel paths, an invalid code, ring reuse and
the documented errors."""
import ctypes as C

import numpy as np
import pytest

import distance_amd as da
import oracle
from closest_reference import bits, cuts_of, plain_truth, special_values_set
from helpers import random_alignment
from links_reference import linked
from tools import synth

pytestmark = pytest.mark.gpu
ALL = ("n", "n_high", "raw", "jc69", "k80", "tn93")
ERR_ARG, ERR_INVALID_CODE, ERR_STATE = 1, 3, 4
L, N_S, MAXREC = 96, 70, 32
INF = float("inf")


@pytest.fixture(scope="module")
def eng():
    e = da.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def data():
    both = random_alignment(2049 + N_S, L, seed=301)
    return both[:2049], both[2049:]


_truth = {}


def truth(eng, tag, measure, streamed, counts=None):
    """the plain stream's S of the set uploaded to slot 0, computed once per (set, measure, flag) and never changed"""
    key = (tag, measure, counts is not None)
    if key not in _truth:
        _truth[key] = plain_truth(eng, measure, streamed, counts, max_records=MAXREC)
    return _truth[key]


def expected(measure, S, Tal, T, values=True, tallies=True):
    """(streamed, loaded[, values][, tallies]) of the links of S[streamed][loaded] at T, streamed outer, loaded inner"""
    n_s, n_l = S.shape
    keep = linked(measure, S.reshape(-1), T)
    i, j = np.divmod(np.arange(n_s * n_l, dtype=np.int64), max(n_l, 1))
    out = (i[keep].astype(np.uint32), j[keep].astype(np.uint32))
    if values:
        out += (S.reshape(-1)[keep],)
    if tallies:
        out += (Tal.reshape(n_s * n_l, -1)[keep],)
    return out


def run_links(eng, measure, T, streamed, cuts, counts=None, max_records=MAXREC, depth=3, nibbles=False, values=True,
              tallies=True, window=0):
    """Push `streamed` cut into batches of the sizes `cuts` through a links stream, popping as the ring fills: the batches'
    links concatenated with the batch's first ordinal added to `streamed`, the links per batch, and stats()."""
    got, firsts, b0 = [], [], 0
    with eng.links_stream(measure, T, max_records, depth=depth, nibbles=nibbles, values=values, tallies=tallies,
                          window=window) as st:
        for size in cuts:
            if st.in_flight() == depth - 1:
                got.append(st.pop())
            st.push(streamed[b0:b0 + size], None if counts is None else counts[b0:b0 + size])
            firsts.append(b0)
            b0 += size
        assert b0 == len(streamed)
        while st.in_flight():
            got.append(st.pop())
        stats = st.stats()
    assert [g[0] for g in got] == list(cuts)
    per_batch = [len(g[1]) for g in got]
    assert stats[0] == sum(per_batch)
    for g, f in zip(got, firsts):
        assert g[1].dtype == np.uint32 and (g[1] < g[0]).all()
    arrays = (np.concatenate([g[1] + np.uint32(f) for g, f in zip(got, firsts)]),)
    arrays += tuple(np.concatenate([g[a] for g in got]) for a in range(2, len(got[0])))
    return arrays, per_batch, stats


def assert_same(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    for n, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, n, g.shape, w.shape, g.dtype, w.dtype)
        assert np.array_equal(bits(g), bits(w)), (what, n)


def status_of(fn, *a, **kw):
    with pytest.raises(da.DistanceError) as e:
        fn(*a, **kw)
    return e.value.status


def median_of(S):
    flat = S.reshape(-1)
    return float(np.median(flat[np.isfinite(flat)] if flat.dtype == np.float64 else flat))


# ---- 1. every measure across the block boundary of a row, and the thresholds ------------------------------------------------
@pytest.mark.parametrize("measure", ALL)
@pytest.mark.parametrize("n_loaded", [1, 2047, 2048, 2049])
def test_every_measure_and_threshold_against_the_plain_stream(eng, data, n_loaded, measure):
    loaded, streamed = data[0][:n_loaded], data[1]
    eng.upload(0, loaded)
    S, Tal = truth(eng, n_loaded, measure, streamed)
    assert S.shape == (N_S, n_loaded)
    if measure in ("n", "n_high", "raw") and n_loaded <= 130:     # the truth itself is pinned
        want = oracle.all_pairs_rect(measure, streamed, loaded)
        want = want.astype(np.int64) if measure in da.INT_MEASURES else want
        assert np.array_equal(bits(S), bits(want)), measure
    cuts = cuts_of(N_S, MAXREC)
    med = median_of(S)
    for T in (-1.0, 0.0, med, INF):
        got, per_batch, stats = run_links(eng, measure, T, streamed, cuts)
        want = expected(measure, S, Tal, T)
        assert_same(got, want, (measure, n_loaded, T))
        assert got[1].dtype == np.uint32 and got[2].dtype == (np.int64 if measure in da.INT_MEASURES else np.float64)
        assert stats == (len(want[0]), 0)                          # every batch fits the default window: nothing late
        if T == -1.0:
            assert len(got[0]) == 0
        if T == INF:
            assert len(got[0]) == int((~np.isnan(S.astype(np.float64))).sum())
    if n_loaded > 1:
        assert 0 < len(expected(measure, S, Tal, med)[0]) < S.size
    if measure in da.INT_MEASURES:                                 # v <= floor(T)
        for T in (2.9, med + 0.9):
            got, _, _ = run_links(eng, measure, T, streamed, cuts)
            assert_same(got, expected(measure, S, Tal, np.floor(T)), (measure, n_loaded, T))
            assert_same(got, run_links(eng, measure, np.floor(T), streamed, cuts)[0], (measure, n_loaded, T, "floor"))
        # a floor below -2^63: nothing can link, and nothing is compacted
        got, per_batch, stats = run_links(eng, measure, -1e30, streamed, cuts)
        assert len(got[0]) == 0 and per_batch == [0, 0, 0] and stats == (0, 0)


# ---- 2. windows --------------------------------------------------------------------------------------------------------------
def test_windows(eng, data):
    loaded, streamed = data[0][:130], data[1]
    eng.upload(0, loaded)
    cuts = cuts_of(N_S, MAXREC)
    for measure, T in (("n", 2), ("k80", 0.03)):
        S, Tal = truth(eng, 130, measure, streamed)
        want = expected(measure, S, Tal, T)
        whole, per_batch, stats = run_links(eng, measure, T, streamed, cuts)
        assert_same(whole, want, measure)
        assert 20 < len(want[0]) < 2000 and min(per_batch) > 5 and stats[1] == 0
        for window in (1, 5):
            got, pb, stats = run_links(eng, measure, T, streamed, cuts, window=window)
            assert_same(got, want, (measure, window))
            assert pb == per_batch
            assert stats == (len(want[0]), sum(-(-n // window) - 1 for n in per_batch if n))   # the late path ran
    # one batch, the window exactly its total, and a larger one: nothing is written after collect
    measure, T = "n", 2
    S, Tal = truth(eng, 130, measure, streamed)
    want = expected(measure, S[:MAXREC], Tal[:MAXREC], T)
    total = len(want[0])
    for window in (total, total + 1, 0):
        got, pb, stats = run_links(eng, measure, T, streamed[:MAXREC], [MAXREC], window=window)
        assert_same(got, want, window)
        assert stats == (total, 0)
    got, pb, stats = run_links(eng, measure, T, streamed[:MAXREC], [MAXREC], window=total - 1)
    assert_same(got, want, "one link short")
    assert stats == (total, 1)


def test_links_batch_at_any_first_link(eng, data):
    loaded, streamed = data[0][:130], data[1]
    eng.upload(0, loaded)
    S, Tal = truth(eng, 130, "raw", streamed)
    T = 0.03
    want = expected("raw", S[:MAXREC], Tal[:MAXREC], T)
    total = len(want[0])
    assert total > 20
    with eng.links_stream("raw", T, MAXREC, tallies=True, window=5) as st:
        st.push(streamed[:MAXREC])
        n, p = C.c_size_t(), C.c_void_p(1)
        assert st._lib.dst_stream_collect(st._h, C.byref(n), C.byref(p)) == 0 and n.value == MAXREC and p.value is None
        assert st.stats() == (total, 0)
        for first in (0, 3, 0, 7, total - 2, total - 5, total, 0):     # unaligned, the short last window, the end, back
            got = st.links_batch(first)
            assert got[0] == total
            m = min(5, total - first)
            assert_same(got[1:], tuple(w[first:first + m] for w in want), first)
        assert st.stats() == (total, 6)                                # window 0 is there after collect; every change since
        assert status_of(st.links_batch, total + 1) == ERR_ARG
        assert st.links_batch(3)[0] == total


# ---- 3. the answer does not depend on the cut ----------------------------------------------------------------------------------
@pytest.mark.parametrize("nibbles", [False, True])
@pytest.mark.parametrize("depth", [2, 3])
def test_every_cut_gives_the_same_bits(eng, data, depth, nibbles):
    loaded, streamed = data[0][:130], data[1]
    eng.upload(0, loaded)
    cuts = [cuts_of(N_S, 1), cuts_of(N_S, 7), cuts_of(N_S, 31), cuts_of(N_S, 32), [32, 5, 1, 32]]
    for measure, T in (("n_high", 3), ("k80", 0.04)):
        S, Tal = truth(eng, 130, measure, streamed)
        want = expected(measure, S, Tal, T)
        assert 20 < len(want[0]) < S.size
        for cut in cuts:
            got, _, _ = run_links(eng, measure, T, streamed, cut, depth=depth, nibbles=nibbles)
            assert_same(got, want, (measure, depth, nibbles, cut[0]))


# ---- 4. special values -------------------------------------------------------------------------------------------------------
def test_special_values(eng):
    base = special_values_set()
    loaded = base[[0, 12, 22, 30, 31, 32]]
    streamed = base
    eng.upload(0, loaded)
    for m in ALL:
        S, Tal = plain_truth(eng, m, streamed, max_records=16)
        res = {}
        for T in (0.0, 0.5, 1e300, INF):
            res[T], _, _ = run_links(eng, m, T, streamed, cuts_of(40, 16), max_records=16)
            assert_same(res[T], expected(m, S, Tal, T), (m, T))
        if m in da.INT_MEASURES:
            continue
        at_inf, at_0 = res[INF], res[0.0]
        assert np.isnan(S).sum() >= 40 + 5 * 5
        assert not np.isnan(at_inf[2]).any() and len(at_inf[0]) == int((~np.isnan(S)).sum())   # NaN never links
        assert not (at_inf[1] == 2).any()                  # the all-N loaded record has no links
        assert len(at_0[0]) >= 10 and (at_0[2] == 0).all()
        if m in ("jc69", "k80"):
            assert np.signbit(at_0[2]).all()               # -k ln(1) = -0.0 links at T = 0, and stays -0.0
        if m == "jc69":                                    # +inf links only at T = inf
            assert np.isposinf(S).sum() >= 10
            assert not np.isinf(res[1e300][2]).any() and int(np.isposinf(at_inf[2]).sum()) == int(np.isposinf(S).sum())


# ---- 5. tn93's counts ----------------------------------------------------------------------------------------------------------
def test_tn93_with_device_counts_and_with_the_callers(eng, data):
    loaded, streamed = data[0][:130], data[1]
    eng.upload(0, loaded)
    counts = oracle.count_bases_matrix(streamed).astype(np.uint32)
    counts[:, 0] += (np.arange(N_S) % 3).astype(np.uint32) * 5      # the caller's counts are the caller's: not the device's
    S0, T0 = truth(eng, 130, "tn93", streamed)
    S1, T1 = truth(eng, 130, "tn93", streamed, counts)
    assert np.array_equal(T0, T1) and not np.array_equal(bits(S0), bits(S1))
    T = median_of(S0)
    cuts = cuts_of(N_S, MAXREC)
    for what in ((True, True), (True, False), (False, True)):
        kw = dict(values=what[0], tallies=what[1])
        got0, _, _ = run_links(eng, "tn93", T, streamed, cuts, **kw)
        got1, _, _ = run_links(eng, "tn93", T, streamed, cuts, counts=counts, **kw)
        assert_same(got0, expected("tn93", S0, T0, T, **kw), what)
        assert_same(got1, expected("tn93", S1, T1, T, **kw), what)
    got0, _, _ = run_links(eng, "tn93", T, streamed, cuts)
    got1, _, _ = run_links(eng, "tn93", T, streamed, cuts, counts=counts)
    assert not (np.array_equal(got0[0], got1[0]) and np.array_equal(bits(got0[2]), bits(got1[2])))


# ---- 6. kernel paths and what ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["low", "random"])
def test_kernel_paths_and_what_give_the_same_bits(kind):
    if kind == "low":
        r = synth.root(synth.SEED, 3000)
        both = synth.records(synth.SEED, r, 0, 130 + 100)
    else:
        both = random_alignment(130 + 100, 3000, seed=311)
    loaded, streamed = both[:130], both[130:]
    whats = [(False, False), (True, False), (False, True), (True, True)]
    with da.Engine(0) as e:
        e.set_prep_threshold(0)
        e.upload(0, loaded)
        e.set_path("dense")
        truths = {m: plain_truth(e, m, streamed, max_records=64) for m in ("raw", "tn93")}
        T = {m: median_of(truths[m][0]) for m in truths}
        got = {}
        for path in ("dense", "consensus", "auto"):
            e.set_path(path)
            for m in ("raw", "tn93"):
                for what in whats:
                    got[path, m, what], _, _ = run_links(e, m, T[m], streamed, cuts_of(100, 64), max_records=64,
                                                         values=what[0], tallies=what[1])
                    if kind == "low" and path != "auto":      # (a low-diversity set is what the lists index: no fall-back)
                        assert e.last_path() == path, (path, m)
        for (path, m, what), g in got.items():
            want = expected(m, *truths[m], T[m], values=what[0], tallies=what[1])
            assert len(g) == 2 + what[0] + what[1] and len(want[0]) > 0
            assert_same(g, want, (kind, path, m, what))


# ---- 7. an invalid code, ring reuse ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nibbles", [False, True])
def test_an_invalid_code_spoils_its_batch_only(eng, data, nibbles):
    loaded, streamed = data[0][:130], data[1]
    eng.upload(0, loaded)
    S, Tal = truth(eng, 130, "raw", streamed)
    T = 0.05
    with eng.links_stream("raw", T, 8, nibbles=nibbles, tallies=True) as st:
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
        first = st.pop()
        assert first[0] == 8
        assert_same(first[1:], expected("raw", S[:8], Tal[:8], T), "the batch before")
        st.push(streamed[12:20])
        with pytest.raises(da.DistanceError) as e:
            st.pop()
        assert e.value.status == ERR_INVALID_CODE and "record 2 at site 6" in e.value.message
        assert status_of(st.links_batch, 0) == ERR_STATE
        third = st.pop()                                         # no poisoning: the next batch is a batch like any other
        assert third[0] == 8 and len(third[1]) > 0
        assert_same(third[1:], expected("raw", S[12:20], Tal[12:20], T), "the batch after")
        assert st.stats() == (len(first[1]) + len(third[1]), 0)
        st.push(streamed[20:28])
        assert_same(st.pop()[1:], expected("raw", S[20:28], Tal[20:28], T), "and the one after that")


@pytest.mark.parametrize("depth", [2, 3])
def test_ring_reuse_with_a_late_window_from_every_batch(eng, data, depth):
    loaded, streamed = data[0][:130], data[1]
    eng.upload(0, loaded)
    S, Tal = truth(eng, 130, "n", streamed)
    T, late = 3, 0
    with eng.links_stream("n", T, 8, depth=depth, tallies=True, window=4) as st:
        for b0 in range(0, 64, 8):                               # eight batches through two or three slots
            st.push(streamed[b0:b0 + 8])
            n, p = C.c_size_t(), C.c_void_p()
            st._eng._check(st._lib.dst_stream_collect(st._h, C.byref(n), C.byref(p)))
            want = expected("n", S[b0:b0 + 8], Tal[b0:b0 + 8], T)
            total = len(want[0])
            assert total > 6, b0
            got = st.links_batch(5)                              # a late window first, then window 0 again
            assert got[0] == total
            assert_same(got[1:], tuple(w[5:9] for w in want), b0)
            assert_same(st.links_batch(0)[1:], tuple(w[:4] for w in want), b0)
            late += 2
            assert st.stats()[1] == late


# ---- 8. the measurement knob: the window by a copy after collect ---------------------------------------------------------------
def test_the_copy_route_gives_the_same_bits(eng, data, monkeypatch):
    loaded, streamed = data[0][:130], data[1]
    eng.upload(0, loaded)
    monkeypatch.setenv("DST_STREAM_LINKS_COPY", "1")
    for measure, T in (("n", 3), ("tn93", 0.04)):
        S, Tal = truth(eng, 130, measure, streamed)
        want = expected(measure, S, Tal, T)
        for window in (0, 5):
            got, per_batch, stats = run_links(eng, measure, T, streamed, cuts_of(N_S, MAXREC), window=window)
            assert_same(got, want, (measure, window))
            assert stats[1] == (sum(-(-n // 5) - 1 for n in per_batch if n) if window else 0)


# ---- 9. misuse: the documented statuses ----------------------------------------------------------------------------------------
def test_misuse(eng, data):
    lib = da.load()
    loaded, streamed = data[0][:130], data[1]
    eng.upload(0, loaded)
    assert status_of(eng.links_stream, 9, 1.0, 8) == ERR_ARG                     # measure
    assert status_of(eng.links_stream, "raw", float("nan"), 8) == ERR_ARG
    assert status_of(eng.links_stream, "raw", 1.0, 8, window=(1 << 22) + 1) == ERR_ARG
    assert status_of(eng.links_stream, "raw", 1.0, 0) == ERR_ARG
    assert status_of(eng.links_stream, "raw", 1.0, 8, depth=1) == ERR_ARG
    assert status_of(eng.links_stream, "raw", 1.0, 8, depth=17) == ERR_ARG
    h = C.c_void_p()
    assert lib.dst_stream_open_links(eng._h, 2, 1.0, 4, 0, 8, 3, 0, C.byref(h)) == ERR_ARG      # unknown bits in what
    assert lib.dst_stream_open_links(eng._h, 2, 1.0, 3, 0, 8, 3, 2, C.byref(h)) == ERR_ARG      # wire
    assert lib.dst_stream_open_links(eng._h, 2, 1.0, 3, 0, 8, 3, 0, None) == ERR_ARG
    assert h.value is None
    with da.Engine(0) as fresh:
        assert status_of(fresh.links_stream, "raw", 1.0, 8) == ERR_STATE         # slot 0 not loaded
    n, total = C.c_uint64(), C.c_uint64()
    sp, lp, vp, tp, ku = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint32()

    def batch(st, *ptrs):
        return lib.dst_stream_links_batch(st._h, 0, *ptrs)

    every = (C.byref(n), C.byref(total), C.byref(sp), C.byref(lp), C.byref(vp), C.byref(tp))
    with eng.links_stream("raw", 0.05, 8, window=1 << 22) as st:                 # the largest window: capped at 8 x 130
        assert batch(st, *every) == ERR_STATE                                    # no collected batch
        st.push(streamed[:8])
        assert batch(st, *every) == ERR_STATE
        got = st.pop()
        for k in range(4):                                                       # a NULL among the four required pointers
            ptrs = list(every)
            ptrs[k] = None
            assert batch(st, *ptrs) == ERR_ARG
        first_total = len(got[1])
        assert batch(st, *every[:4], None, None) == 0 and n.value == first_total == total.value
        assert batch(st, *every) == 0 and vp.value is not None and tp.value is None          # tallies were not asked for
        index = np.zeros(650, np.uint32)
        assert lib.dst_stream_closest_batch(st._h, C.byref(sp), C.byref(tp), C.byref(vp), C.byref(ku)) == ERR_ARG
        assert lib.dst_stream_closest_result(st._h, index.ctypes.data, None, None, 650, C.byref(ku)) == ERR_ARG
        assert lib.dst_stream_closest_next_index(st._h, 5) == ERR_ARG
        st.push(streamed[8:16])                                                  # the next submit ends the batch's validity
        assert batch(st, *every) == ERR_STATE
        st.pop()
        eng.upload(0, loaded[:100])                                              # the loaded set's record count changed
        assert status_of(st.push, streamed[:8]) == ERR_STATE
    eng.upload(0, loaded)
    with eng.links_stream("raw", 0.05, 8, values=False) as st:                   # what == 0
        st.push(streamed[:8])
        got = st.pop()
        assert len(got) == 3 and len(got[1]) == first_total > 0
        assert batch(st, *every) == 0 and total.value == first_total and vp.value is None and tp.value is None
    for other in (eng.stream("raw", max_records=8, depth=2), eng.closest_stream("raw", 5, 8),
                  eng.closest_stream("raw", 5, 8, side="streamed")):
        with other as st:
            assert batch(st, *every) == ERR_ARG
            assert lib.dst_stream_links_stats(st._h, C.byref(n), C.byref(total)) == ERR_ARG


# ---- 10. the context's other calls afterwards ----------------------------------------------------------------------------------
def test_a_plain_stream_and_links_afterwards(data):
    loaded, streamed = data[0][:130], data[1]
    with da.Engine(0) as e:
        e.upload(0, loaded)
        before = plain_truth(e, "tn93", streamed, max_records=MAXREC)
        links_before = e.links("tn93", 0.05, tallies=True)
        e.upload(1, streamed)
        rect_before = e.links("n", 3, square=False, row_slot=1, col_slot=0, tallies=True)
        want = expected("tn93", *before, 0.05)
        for window in (0, 7):
            got, _, _ = run_links(e, "tn93", 0.05, streamed, cuts_of(N_S, MAXREC), window=window)
            assert_same(got, want, window)
        after = plain_truth(e, "tn93", streamed, max_records=MAXREC)
        assert_same(after, before, "the plain stream")
        assert_same(e.links("tn93", 0.05, tallies=True), links_before, "links, square")
        assert_same(e.links("n", 3, square=False, row_slot=1, col_slot=0, tallies=True), rect_before, "links, rectangle")
        # the stream's rectangle is dst_links' rectangle with the batch as rows
        S, Tal = plain_truth(e, "n", streamed, max_records=MAXREC)
        assert_same(rect_before, expected("n", S, Tal, 3), "dst_links and the stream agree")
