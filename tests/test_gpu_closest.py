"""GPU (-m gpu): closest streams (dst_stream_open_closest / Engine.closest_stream) — the k nearest records kept on the GPU
while a stream goes past — against the plain stream's own results of the same batches, bit for bit: every measure, the
list-slot boundaries of k, last column blocks of 1 and 2, every cut of the stream, ties, NaN / +inf / -0.0, the kernel
paths, the ends of the ordinal range, snapshots, the per-batch side, and the documented errors."""
import ctypes as C

import numpy as np
import pytest

import distance_amd as da
import oracle
from closest_reference import (assert_same, bits, cuts_of, expected_for_loaded, expected_for_streamed, plain_truth, run_closest,
                               special_values_set)
from helpers import random_alignment
from tools import synth

pytestmark = pytest.mark.gpu
ALL = ("n", "n_high", "raw", "jc69", "k80", "tn93")
KS = (1, 5, 64, 65, 256)            # the slot boundaries of the wave-resident list
ERR_ARG, ERR_INVALID_CODE, ERR_STATE, ERR_CAPACITY = 1, 3, 4, 6
L, N_S, MAXREC = 300, 333, 200


@pytest.fixture(scope="module")
def eng():
    e = da.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def data():
    return random_alignment(130, L, seed=101), random_alignment(N_S, L, seed=102)


_truth = {}


def truth(eng, tag, measure, streamed, counts=None):
    """the plain stream's S of the set uploaded to slot 0, computed once per (set, measure, flag) and never changed"""
    key = (tag, measure, counts is not None)
    if key not in _truth:
        _truth[key] = plain_truth(eng, measure, streamed, counts, max_records=MAXREC)
    return _truth[key]


def status_of(fn, *a, **kw):
    with pytest.raises(da.DistanceError) as e:
        fn(*a, **kw)
    return e.value.status


# ---- 1. shapes: every measure, k at the slot boundaries, last column blocks of 1 and 2 ----------------------------------
@pytest.mark.parametrize("measure", ALL)
@pytest.mark.parametrize("n_loaded", [1, 64, 65, 130])
def test_every_measure_and_k_against_the_plain_stream(eng, data, n_loaded, measure):
    loaded, streamed = data[0][:n_loaded], data[1]
    eng.upload(0, loaded)
    S, T = truth(eng, n_loaded, measure, streamed)
    assert S.shape == (N_S, n_loaded)
    if measure in ("n", "n_high", "raw"):     # the truth itself is pinned
        want = oracle.all_pairs_rect(measure, streamed, loaded)
        want = want.astype(np.int64) if measure in da.INT_MEASURES else want
        assert np.array_equal(bits(S), bits(want)), measure
    for k in KS:
        got = run_closest(eng, measure, k, streamed, cuts_of(N_S, MAXREC), max_records=MAXREC)
        assert got[0].shape == (n_loaded, k) and got[1].dtype == (np.int64 if measure in da.INT_MEASURES else np.float64)
        assert_same(got, expected_for_loaded(S, T, k), (measure, n_loaded, k))


def test_tn93_with_device_counts_and_with_the_callers(eng, data):
    loaded, streamed = data
    eng.upload(0, loaded)
    counts = oracle.count_bases_matrix(streamed).astype(np.uint32)
    counts[:, 0] += (np.arange(N_S) % 3).astype(np.uint32) * 5      # the caller's counts are the caller's: not the device's
    S0, T0 = truth(eng, 130, "tn93", streamed)
    S1, T1 = truth(eng, 130, "tn93", streamed, counts)
    assert np.array_equal(T0, T1) and not np.array_equal(bits(S0), bits(S1))
    for k in (5, 65):
        assert_same(run_closest(eng, "tn93", k, streamed, cuts_of(N_S, 64), max_records=MAXREC), expected_for_loaded(S0, T0, k))
        assert_same(run_closest(eng, "tn93", k, streamed, cuts_of(N_S, 64), counts=counts, max_records=MAXREC),
                    expected_for_loaded(S1, T1, k))


# ---- 2. the answer does not depend on the cut ------------------------------------------------------------------------------
@pytest.mark.parametrize("nibbles", [False, True])
@pytest.mark.parametrize("depth", [2, 3])
def test_every_cut_gives_the_same_bits(eng, data, depth, nibbles):
    loaded, streamed = data
    eng.upload(0, loaded)
    cuts = [cuts_of(N_S, 1), cuts_of(N_S, 7), cuts_of(N_S, 63), cuts_of(N_S, 64), cuts_of(N_S, 65), [200, 133]]
    for measure in ("n_high", "k80"):
        want = expected_for_loaded(*truth(eng, 130, measure, streamed), 65)
        for cut in cuts:
            got = run_closest(eng, measure, 65, streamed, cut, max_records=MAXREC, depth=depth, nibbles=nibbles)
            assert_same(got, want, (measure, depth, nibbles, cut[0]))


# ---- 3. ties and special values ----------------------------------------------------------------------------------------------
def test_ties_resolve_by_ordinal_and_specials_sort_last(eng):
    base = special_values_set()
    loaded = base[[0, 12, 22, 30, 31, 32]]
    # duplicates within a batch, across batches (16 records each) and of loaded records; five all-N records, twice
    streamed = np.concatenate([base, base[::-1], base[5:15]])
    n_s = len(streamed)
    eng.upload(0, loaded)
    for m in ALL:
        S, T = plain_truth(eng, m, streamed, max_records=16)
        for k in (5, 64, 256):
            got = run_closest(eng, m, k, streamed, cuts_of(n_s, 16), max_records=16)
            assert got[0].shape == (6, min(k, n_s))          # k_used = min(k, records streamed): no sentinel entry
            assert_same(got, expected_for_loaded(S, T, k), (m, k))
            assert (got[0] < n_s).all()
        if m in da.INT_MEASURES:
            continue
        # column 0, a copy of the root: zeros first (distance 0 is a neighbour) in ordinal order, then the finite values,
        # the infinities, and the NaNs of the all-N records last
        col = S[:, 0]
        zeros, infs, nans = (np.nonzero(f(col))[0] for f in (lambda x: x == 0, np.isposinf, np.isnan))
        assert len(zeros) == 25 and len(nans) >= 10 and (m != "jc69" or len(infs) == 25), (m, len(zeros), len(infs), len(nans))
        idx, vals, _ = got
        assert list(idx[0][:25]) == list(zeros) and (vals[0][:25] == 0).all(), m
        assert list(idx[0][n_s - len(nans):]) == list(nans) and np.isnan(vals[0][n_s - len(nans):]).all(), m
        at = n_s - len(nans) - len(infs)
        assert list(idx[0][at:at + len(infs)]) == list(infs) and np.isposinf(vals[0][at:at + len(infs)]).all(), m
        assert np.isfinite(vals[0][:at]).all()
        if m in ("jc69", "k80"):
            assert np.signbit(vals[0][:25]).all()             # -k ln(1) = -0.0: the key of +0.0, and it stays -0.0
        # an all-N loaded record (column 2): every value NaN, so the order is the ordinals'
        assert np.isnan(vals[2]).all() and list(idx[2]) == list(range(n_s)), m


def test_fewer_records_than_k(eng, data):
    loaded, streamed = data
    eng.upload(0, loaded)
    with eng.closest_stream("raw", 5, 8) as st:
        idx, vals = st.result()
        assert idx.shape == (130, 0) and vals.shape == (130, 0)
        st.push(streamed[:3])
        assert st.pop() == 3
        idx, vals, tal = st.result(tallies=True)
    S, T = truth(eng, 130, "raw", streamed)
    assert idx.shape == (130, 3) and tal.shape == (130, 3, 2)
    assert_same((idx, vals, tal), expected_for_loaded(S[:3], T[:3], 5))


# ---- 4. kernel paths ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["low", "random"])
def test_kernel_paths_give_the_same_bits(kind):
    if kind == "low":
        r = synth.root(synth.SEED, 3000)
        both = synth.records(synth.SEED, r, 0, 130 + 200)
    else:
        both = random_alignment(130 + 200, 3000, seed=111)
    loaded, streamed = both[:130], both[130:]
    with da.Engine(0) as e:
        e.set_prep_threshold(0)
        e.upload(0, loaded)
        got = {}
        for path in ("dense", "consensus", "auto"):
            e.set_path(path)
            for m in ("raw", "tn93"):
                got[path, m] = run_closest(e, m, 10, streamed, cuts_of(200, 64), max_records=64)
                if kind == "low" and path != "auto":      # (a low-diversity set is what the lists index: no fall-back)
                    assert e.last_path() == path, (path, m)
        e.set_path("dense")
        for m in ("raw", "tn93"):
            want = expected_for_loaded(*plain_truth(e, m, streamed, max_records=64), 10)
            for path in ("dense", "consensus", "auto"):
                assert_same(got[path, m], want, (kind, path, m))


# ---- 5. ordinals ---------------------------------------------------------------------------------------------------------------
def test_ordinals_compare_unsigned_across_2_31(eng, data):
    loaded, streamed = data[0], data[1][:12].copy()
    streamed[:] = streamed[0]                                  # twelve copies: every key ties, the ordinal decides
    eng.upload(0, loaded)
    S, T = plain_truth(eng, "raw", streamed, max_records=4)
    first = 2**31 - 3
    got = run_closest(eng, "raw", 8, streamed, [4, 4, 4], max_records=4, first_index=first)
    assert_same(got, expected_for_loaded(S, T, 8, ordinals=first + np.arange(12)))
    assert list(got[0][0]) == [first + i for i in range(8)]    # 2^31 - 3 .. 2^31 + 4, ascending as unsigned


def test_ordinals_end_at_2_32_minus_2(eng, data):
    loaded, streamed = data
    eng.upload(0, loaded)
    S, T = truth(eng, 130, "raw", streamed)
    first = 2**32 - 70
    with eng.closest_stream("raw", 5, 64) as st:
        st.next_index(first)
        st.push(streamed[:64])
        assert st.pop() == 64
        before = st.result(tallies=True)
        assert_same(before, expected_for_loaded(S[:64], T[:64], 5, ordinals=first + np.arange(64)))
        assert int(before[0].max()) <= 2**32 - 7
        assert status_of(st.push, streamed[64:74]) == ERR_CAPACITY        # 2^32 - 6 + 9 passes 2^32 - 2
        assert st.in_flight() == 0
        assert_same(st.result(tallies=True), before)


def test_next_index_misuse(eng, data):
    loaded, streamed = data
    eng.upload(0, loaded)
    with eng.closest_stream("raw", 5, 64) as st:
        st.next_index(100)
        assert status_of(st.next_index, 99) == ERR_ARG                   # backwards
        st.push(streamed[:10])
        assert status_of(st.next_index, 1000) == ERR_STATE               # a batch in flight
        st.pop()
        assert status_of(st.next_index, 109) == ERR_ARG                  # ten records went by
        st.next_index(110)
        idx, _ = st.result()
        assert idx.min() >= 100 and idx.max() <= 109 and idx.shape == (130, 5)


# ---- 6. snapshots, and other work on the context in between --------------------------------------------------------------
def test_snapshot_and_other_calls_in_between(eng, data):
    loaded, streamed = data
    eng.upload(0, loaded)
    S, T = truth(eng, 130, "tn93", streamed)
    whole = run_closest(eng, "tn93", 65, streamed, cuts_of(N_S, 64), max_records=64)
    sq = eng.run_square("raw")
    with eng.closest_stream("tn93", 65, 64) as st:
        for b0 in (0, 64, 128):
            st.push(streamed[b0:b0 + 64])
            st.pop()
        half = st.result(tallies=True)
        assert_same(half, expected_for_loaded(S[:192], T[:192], 65), "half")
        idx, _ = eng.nearest("raw", 3)
        assert idx.shape == (130, 3)
        assert np.array_equal(bits(eng.run_square("raw")), bits(sq))
        assert_same(st.result(tallies=True), half, "a snapshot twice")
        for b0 in (192, 256, 320):
            st.push(streamed[b0:b0 + 64])
            st.pop()
        assert_same(st.result(tallies=True), whole, "after the rest")
    assert_same(whole, expected_for_loaded(S, T, 65))


# ---- 7. side="streamed": dst_nearest's rectangle form per batch ----------------------------------------------------------
@pytest.mark.parametrize("n_loaded", [1, 65, 700])
def test_streamed_side_equals_nearest_per_batch(eng, n_loaded):
    loaded = random_alignment(n_loaded, L, seed=121)
    streamed = random_alignment(150, L, seed=122)
    cuts = cuts_of(150, 64)
    eng.upload(0, loaded)
    for m in ALL:
        S, T = plain_truth(eng, m, streamed, max_records=64)
        for k in (1, 5, 65, 256):
            ku = min(k, n_loaded)
            want = []
            for b0 in range(0, 150, 64):
                eng.upload(1, streamed[b0:b0 + 64])
                want.append(eng.nearest(m, k, square=False, row_slot=1, col_slot=0, tallies=True))
            got = run_closest(eng, m, k, streamed, cuts, max_records=64, side="streamed")
            assert got[0].shape == (150, ku), (m, k)
            assert np.array_equal(got[0], np.concatenate([w[0] for w in want])), (m, k)
            assert np.array_equal(got[2], np.concatenate([w[2] for w in want])), (m, k)
            assert_same(got, expected_for_streamed(S, T, k), (m, k))     # values: the plain stream's bits


# ---- 8. misuse: the documented statuses ----------------------------------------------------------------------------------
def test_misuse(eng, data):
    lib = da.load()
    loaded, streamed = data
    eng.upload(0, loaded)
    assert status_of(eng.closest_stream, "raw", 0, 8) == ERR_ARG
    assert status_of(eng.closest_stream, "raw", 257, 8) == ERR_ARG
    assert status_of(eng.closest_stream, "raw", 5, 8, side=2) == ERR_ARG
    assert status_of(eng.closest_stream, "raw", 5, 8, side="both") == ERR_ARG
    assert status_of(eng.closest_stream, "raw", 5, 0) == ERR_ARG
    assert status_of(eng.closest_stream, "raw", 5, 8, depth=1) == ERR_ARG
    assert status_of(eng.closest_stream, "raw", 5, 8, depth=17) == ERR_ARG
    with da.Engine(0) as fresh:
        assert status_of(fresh.closest_stream, "raw", 5, 8) == ERR_STATE       # slot 0 not loaded
    ip, tp, vp, ku = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint32()
    with eng.closest_stream("raw", 5, 8) as st:
        st.push(streamed[:8])
        assert status_of(st.result) == ERR_STATE                               # a batch in flight
        n, p = C.c_size_t(), C.c_void_p(1)
        assert lib.dst_stream_collect(st._h, C.byref(n), C.byref(p)) == 0 and n.value == 8 and p.value is None
        assert status_of(st.result, cap_entries=130 * 5 - 1) == ERR_CAPACITY
        assert st.result()[0].shape == (130, 5)
        assert lib.dst_stream_closest_batch(st._h, C.byref(ip), C.byref(tp), C.byref(vp), C.byref(ku)) == ERR_ARG
    with eng.closest_stream("raw", 5, 8, side="streamed") as st:
        assert status_of(st.result) == ERR_ARG
        assert status_of(st.next_index, 5) == ERR_ARG
        st.push(streamed[:8])
        idx, vals, tal = st.pop()
        assert idx.shape == (8, 5) and vals.shape == (8, 5) and tal.shape == (8, 5, 2)
    with eng.stream("raw", max_records=8, depth=2) as st:
        index = np.zeros(650, np.uint32)
        assert lib.dst_stream_closest_batch(st._h, C.byref(ip), C.byref(tp), C.byref(vp), C.byref(ku)) == ERR_ARG
        assert lib.dst_stream_closest_result(st._h, index.ctypes.data, None, None, 650, C.byref(ku)) == ERR_ARG
        assert lib.dst_stream_closest_next_index(st._h, 5) == ERR_ARG


@pytest.mark.parametrize("nibbles", [False, True])
def test_an_invalid_code_poisons_the_lists(eng, data, nibbles):
    loaded, streamed = data
    eng.upload(0, loaded)
    with eng.closest_stream("raw", 5, 8, nibbles=nibbles) as st:
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
