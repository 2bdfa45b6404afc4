"""GPU (-m gpu): group-summary streams (dst_stream_open_group_summary / Engine.group_summary_stream) - dst_group_summary on
the rectangle (every record streamed so far) x (the loaded set) - against the plain stream's own matrix S[streamed][loaded]
of the same records reduced by the numpy restatement of dst_group_summary's definition (group_summary_reference, rectangle
form): S for the cells and the streamed side, S.T with the label arrays swapped for the loaded side.  Integers are compared
for equality and doubles bitwise; there is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import distance_amd as da
import oracle
from closest_reference import bits, cuts_of, plain_truth, special_values_set
from group_summary_reference import CELL_KEYS, REC_KEYS, assert_group_summary, check_consequences, group_summary
from helpers import alignment_root, random_alignment
from summary_reference import assert_summary
from tools import synth

pytestmark = pytest.mark.gpu
ALL = ("n", "n_high", "raw", "jc69", "k80", "tn93")
ERR_ARG, ERR_INVALID_CODE, ERR_STATE, ERR_CAPACITY = 1, 3, 4, 6
R, COLS = da._lib.STREAM_GROUPS_ROWS, da._lib.STREAM_GROUPS_COLS
NONE = da._lib.GROUP_NONE
L, N_S, MAXREC, N_L = 96, 70, 32, 2 * COLS + 1
INF = float("inf")
WHATS = [(False, False), (True, False), (False, True), (True, True)]   # (loaded, streamed)


@pytest.fixture(scope="module")
def eng():
    e = da.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def data():
    """513 loaded and 70 streamed records of one alignment; every 41st record is far from the rest (the root's complement),
    so jc69 / k80 saturate (the summary stream test's fixture)"""
    both = random_alignment(N_L + N_S, L, seed=401)
    root = alignment_root(L, 401)
    alt = np.array([{136: 72, 72: 136, 40: 24, 24: 40}[int(c)] for c in root], np.uint8)
    far = random_alignment(64, L, seed=402, root=alt)
    both[5::41] = far[:len(both[5::41])]
    return both[:N_L], both[N_L:]


_truth = {}


def truth(eng, tag, measure, streamed, counts=None):
    """the plain stream's S of the set uploaded to slot 0, computed once per (set, measure, flag) and never changed"""
    key = (tag, measure, counts is not None)
    if key not in _truth:
        _truth[key] = plain_truth(eng, measure, streamed, counts, max_records=MAXREC)[0]
    return _truth[key]


def labels(n, G, layout, seed=0):
    """uint32 labels of n records in G groups: contiguous runs, interleaved record by record, or random with unassigned ones"""
    if layout == "contiguous":
        g = (np.arange(n, dtype=np.int64) * G) // max(n, 1)
    elif layout == "interleaved":
        g = np.arange(n, dtype=np.int64) % G
    elif layout == "none":
        g = np.full(n, NONE, np.int64)
    else:
        rng = np.random.default_rng(seed)
        g = rng.integers(0, G, n)
        g[rng.random(n) < 0.15] = NONE
    return g.astype(np.uint32)


def reference(measure, S, T, lg, Gl, sg, Gs):
    """(what result() must return with loaded=True, what the batches' streamed side must be) from S; None labels: group 0"""
    n_s, n_l = S.shape
    lg = np.zeros(n_l, np.uint32) if lg is None else lg
    sg = np.zeros(n_s, np.uint32) if sg is None else sg
    rows = group_summary(measure, S, n_s, n_l, False, T, sg, Gs, lg, Gl)
    cols = group_summary(measure, np.ascontiguousarray(S.T), n_l, n_s, False, T, lg, Gl, sg, Gs)
    for key in CELL_KEYS:
        assert np.array_equal(bits(rows[key]), bits(cols[key].T)), key      # the reference agrees with itself
    want = {k: rows[k] for k in CELL_KEYS}
    want.update({k: cols[k] for k in REC_KEYS}, records=n_s)
    return want, tuple(rows[k] for k in REC_KEYS)


def run_groups(eng, measure, streamed, cuts, lg, Gl, sg, Gs, T=INF, loaded=False, streamed_side=False, counts=None,
               max_records=MAXREC, depth=3, nibbles=False):
    """Push `streamed` cut into batches of the sizes `cuts` through a group-summary stream, popping as the ring fills:
    result() and the batches' streamed side concatenated (None without it)."""
    got, b0 = [], 0
    with eng.group_summary_stream(measure, max_records, loaded_groups=lg, n_loaded_groups=Gl, n_streamed_groups=Gs,
                                  threshold=T, loaded=loaded, streamed=streamed_side, depth=depth, nibbles=nibbles) as st:
        for size in cuts:
            if st.in_flight() == depth - 1:
                got.append(st.pop())
            st.push(streamed[b0:b0 + size], None if counts is None else counts[b0:b0 + size],
                    None if sg is None else sg[b0:b0 + size])
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
    res, side = got
    want_res, want_side = want
    assert res["records"] == want_res["records"], what
    assert ("rec_within" in res) == ("rec_summable" in res) == ("rec_sum" in res), what
    assert_group_summary(res, want_res, what)
    if side is not None:
        assert side[0].dtype == np.uint32 and side[1].dtype == np.uint32 and side[2].dtype == np.float64, what
        for a, name in enumerate(REC_KEYS):
            assert side[a].shape == want_side[a].shape, (what, name, side[a].shape)
            assert np.array_equal(bits(side[a]), bits(want_side[a])), (what, "streamed", name)


def check_empty_rules(measure, res):
    """the reference's empty-cell rule on a result: a cell without a pair that is not NaN reports the quiet NaN, or 0"""
    empty = res["pairs"] == res["nan_pairs"]
    if measure in da.INT_MEASURES:
        assert (res["min"][empty] == 0).all() and (res["max"][empty] == 0).all()
    else:
        assert (bits(res["min"])[empty] == 0x7FF8000000000000).all() and (bits(res["max"])[empty] == 0x7FF8000000000000).all()
        assert not np.isnan(res["min"][~empty]).any()


def status_of(fn, *a, **kw):
    with pytest.raises(da.DistanceError) as e:
        fn(*a, **kw)
    return e.value.status


def median_of(S):
    flat = S.reshape(-1)
    return float(np.median(flat[np.isfinite(flat)] if flat.dtype == np.float64 else flat))


# ---- 1. every measure x what across the tile's column boundaries -------------------------------------------------------------
@pytest.mark.parametrize("measure", ALL)
@pytest.mark.parametrize("n_loaded", [1, COLS - 1, COLS, COLS + 1, 2 * COLS + 1])
def test_every_measure_and_what_against_the_plain_stream(eng, data, n_loaded, measure):
    loaded, streamed = data[0][:n_loaded], data[1]
    eng.upload(0, loaded)
    S = truth(eng, n_loaded, measure, streamed)
    assert S.shape == (N_S, n_loaded)
    if measure in ("n", "n_high", "raw") and n_loaded <= COLS:     # the truth itself is pinned
        want = oracle.all_pairs_rect(measure, streamed, loaded)
        want = want.astype(np.int64) if measure in da.INT_MEASURES else want
        assert np.array_equal(bits(S), bits(want)), measure
    lg, sg = labels(n_loaded, 3, "random", 1), labels(N_S, 3, "random", 2)
    T = median_of(S)
    want = reference(measure, S, T, lg, 3, sg, 3)
    for lo, st in WHATS:
        got = run_groups(eng, measure, streamed, cuts_of(N_S, MAXREC), lg, 3, sg, 3, T, loaded=lo, streamed_side=st)
        assert ("rec_within" in got[0]) == lo and (got[1] is not None) == st
        check(got, want, (measure, n_loaded, lo, st))
    check_empty_rules(measure, want[0])
    if n_loaded > 1:
        assert 0 < int(want[0]["links"].sum()) < int(want[0]["pairs"].sum())


# ---- 1b. the tile's rows ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", ["n", "k80"])
def test_tile_rows(eng, data, measure):
    sizes = [1, R - 1, R, R + 1]
    streamed = random_alignment(sum(sizes), L, seed=411)
    eng.upload(0, data[0][:COLS + 1])
    S = plain_truth(eng, measure, streamed, max_records=R + 1)[0]
    T = median_of(S)
    for layout in ("interleaved", "contiguous", "random"):
        lg, sg = labels(COLS + 1, 3, layout, 3), labels(len(streamed), 3, layout, 4)
        got = run_groups(eng, measure, streamed, sizes, lg, 3, sg, 3, T, loaded=True, streamed_side=True, max_records=R + 1)
        check(got, reference(measure, S, T, lg, 3, sg, 3), (measure, layout))


# ---- 2. the group counts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Gl", [1, 2, 3, 64, 65, 1024])
def test_group_counts(eng, data, Gl):
    loaded, streamed = data[0][:COLS + 1], data[1]
    eng.upload(0, loaded)
    S = truth(eng, COLS + 1, "raw", streamed)
    T = median_of(S)
    lg = labels(COLS + 1, Gl, "interleaved")
    for Gs in (1, 2, 3, 64, 65, 1024):
        sg = labels(N_S, Gs, "interleaved")
        got = run_groups(eng, "raw", streamed, cuts_of(N_S, MAXREC), lg, Gl, sg, Gs, T, loaded=True, streamed_side=True)
        want = reference("raw", S, T, lg, Gl, sg, Gs)
        check(got, want, (Gl, Gs))
        assert got[0]["pairs"].shape == (Gs, Gl) and got[0]["rec_sum"].shape == (COLS + 1, Gs) and got[1][0].shape == (N_S, Gl)
        check_empty_rules("raw", got[0])


# ---- 3. label layouts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", ["n_high", "jc69"])
def test_label_layouts(eng, data, measure):
    loaded, streamed = data[0][:COLS + 1], data[1]
    n_l = COLS + 1
    eng.upload(0, loaded)
    S = truth(eng, n_l, measure, streamed)
    T = median_of(S)
    one_out_l, one_out_s = labels(n_l, 3, "interleaved"), labels(N_S, 3, "interleaved")
    one_out_l[100] = NONE
    one_out_s[33] = NONE
    hole_l, hole_s = labels(n_l, 2, "contiguous") * 2, labels(N_S, 2, "interleaved") * 2     # group 1 of 4 has no member, nor 3
    layouts = {"contiguous": (labels(n_l, 3, "contiguous"), 3, labels(N_S, 3, "contiguous"), 3),
               "interleaved": (labels(n_l, 3, "interleaved"), 3, labels(N_S, 3, "interleaved"), 3),
               "no loaded record assigned": (labels(n_l, 3, "none"), 3, labels(N_S, 3, "interleaved"), 3),
               "no streamed record assigned": (labels(n_l, 3, "interleaved"), 3, labels(N_S, 3, "none"), 3),
               "one unassigned record": (one_out_l, 3, one_out_s, 3),
               "a group with no member": (hole_l, 4, hole_s, 4),
               "labels omitted": (None, 1, None, 1),
               "streamed labels omitted": (labels(n_l, 3, "contiguous"), 3, None, 2)}
    for name, (lg, Gl, sg, Gs) in layouts.items():
        want = reference(measure, S, T, lg, Gl, sg, Gs)
        for lo, st in WHATS:
            check(run_groups(eng, measure, streamed, cuts_of(N_S, MAXREC), lg, Gl, sg, Gs, T, loaded=lo, streamed_side=st),
                  want, (measure, name, lo, st))
        check_empty_rules(measure, want[0])
    # every record has a row, assigned or not
    want = reference(measure, S, INF, layouts["no streamed record assigned"][0], 3, labels(N_S, 3, "none"), 3)
    assert int(want[0]["pairs"].sum()) == 0 and int(want[1][1].sum()) > 0 and int(want[0]["rec_summable"].sum()) == 0
    want = reference(measure, S, INF, labels(n_l, 3, "none"), 3, labels(N_S, 3, "interleaved"), 3)
    assert int(want[0]["pairs"].sum()) == 0 and int(want[1][1].sum()) == 0 and int(want[0]["rec_summable"].sum()) > 0


# ---- 4. the answer does not depend on the cut, the depth or the wire ----------------------------------------------------------
@pytest.mark.parametrize("nibbles", [False, True])
@pytest.mark.parametrize("depth", [2, 3])
def test_every_cut_gives_the_same_bits(eng, data, depth, nibbles):
    loaded, streamed = data[0][:COLS + 1], data[1]
    eng.upload(0, loaded)
    lg, sg = labels(COLS + 1, 3, "random", 5), labels(N_S, 65, "random", 6)
    for measure in ("n_high", "k80"):
        S = truth(eng, COLS + 1, measure, streamed)
        T = median_of(S)
        want = reference(measure, S, T, lg, 3, sg, 65)
        for cut in (cuts_of(N_S, MAXREC), [N_S], cuts_of(N_S, 1), [32, 5, 1, 32]):
            got = run_groups(eng, measure, streamed, cut, lg, 3, sg, 65, T, loaded=True, streamed_side=True,
                             max_records=max(cut), depth=depth, nibbles=nibbles)
            check(got, want, (measure, depth, nibbles, cut[0]))


# ---- 5. special values -------------------------------------------------------------------------------------------------------
def test_special_values(eng):
    base = special_values_set()
    loaded = base[[0, 12, 22, 30, 31, 32, 1]]              # a root, a saturated one, all N, three ordinary, the root again
    streamed = base
    lg = np.array([0, 1, 2, 0, 1, 0, 0], np.uint32)
    sg = (np.arange(40) // 5 % 4).astype(np.uint32)        # roots 0 1, saturated 2 3, all N 0, ordinary 1 2 3
    eng.upload(0, loaded)
    for m in ALL:
        S = plain_truth(eng, m, streamed, max_records=16)[0]
        finite = S[np.isfinite(S)] if S.dtype == np.float64 else S.reshape(-1)
        med = float(np.median(finite))
        below = float(finite[finite < med].max()) if (finite < med).any() else med - 1
        res = {}
        for T in (below, med, float(np.nextafter(med, INF)) if m not in da.INT_MEASURES else med + 1, 1e300, INF, 0.0):
            want = reference(m, S, T, lg, 3, sg, 4)
            res[T] = run_groups(eng, m, streamed, cuts_of(40, 16), lg, 3, sg, 4, T, loaded=True, streamed_side=True, max_records=16)
            check(res[T], want, (m, T))
            check_empty_rules(m, res[T][0])
        at_0, at_inf = res[0.0][0], res[INF][0]
        assert int(at_0["links"][0, 0]) >= 5 * 2 and at_0["rec_within"][0, 0] >= 5      # duplicates link at T = 0
        if m in da.INT_MEASURES:
            continue
        # raw NaN: an all-N record on either side is summable with nobody and links with nobody; cell (*, 2) is all NaN
        assert int(at_inf["nan_pairs"].sum()) == int(np.isnan(S).sum()) >= 40 + 5 * 6
        assert (at_inf["nan_pairs"][:, 2] == at_inf["pairs"][:, 2]).all() and np.isnan(at_inf["min"][:, 2]).all()
        assert not at_inf["rec_summable"][2].any() and not res[INF][1][1][20:25].any()
        if m == "jc69":                                    # +inf links only at T = inf and is not summable
            n_inf = int(np.isposinf(S).sum())
            assert n_inf >= 10 and np.isposinf(at_inf["max"]).any()
            assert int(at_inf["links"].sum()) - int(res[1e300][0]["links"].sum()) == n_inf
        if m == "raw":                                     # 0.75 2^37 is above 2^32: both words of the sums are in use
            assert S[np.isfinite(S)].max() >= 0.7 and at_inf["sum"].max() > 5.0


# ---- 6. tn93's counts ----------------------------------------------------------------------------------------------------------
def test_tn93_with_device_counts_and_with_the_callers(eng, data):
    loaded, streamed = data[0][:COLS + 1], data[1]
    eng.upload(0, loaded)
    counts = oracle.count_bases_matrix(streamed).astype(np.uint32)
    counts[:, 0] += (np.arange(N_S) % 3).astype(np.uint32) * 5      # the caller's counts are the caller's: not the device's
    S0 = truth(eng, COLS + 1, "tn93", streamed)
    S1 = truth(eng, COLS + 1, "tn93", streamed, counts)
    assert not np.array_equal(bits(S0), bits(S1))
    T = median_of(S0)
    lg, sg = labels(COLS + 1, 3, "random", 7), labels(N_S, 2, "random", 8)
    cuts = cuts_of(N_S, MAXREC)
    got0 = run_groups(eng, "tn93", streamed, cuts, lg, 3, sg, 2, T, loaded=True, streamed_side=True)
    got1 = run_groups(eng, "tn93", streamed, cuts, lg, 3, sg, 2, T, loaded=True, streamed_side=True, counts=counts)
    check(got0, reference("tn93", S0, T, lg, 3, sg, 2), "device counts")
    check(got1, reference("tn93", S1, T, lg, 3, sg, 2), "caller's counts")
    assert not np.array_equal(bits(got0[0]["sum"]), bits(got1[0]["sum"]))


# ---- 7. kernel paths -----------------------------------------------------------------------------------------------------------
def test_kernel_paths_give_the_same_bits():
    r = synth.root(synth.SEED, 3000)
    both = synth.records(synth.SEED, r, 0, 130 + 100)
    loaded, streamed = both[:130], both[130:]
    lg, sg = labels(130, 3, "random", 9), labels(100, 3, "random", 10)
    with da.Engine(0) as e:
        e.set_prep_threshold(0)
        e.upload(0, loaded)
        e.set_path("dense")
        truths = {m: plain_truth(e, m, streamed, max_records=64)[0] for m in ("raw", "tn93")}
        results = {}
        for path in ("dense", "consensus"):
            e.set_path(path)
            for m in ("raw", "tn93"):
                T = median_of(truths[m])
                got = run_groups(e, m, streamed, cuts_of(100, 64), lg, 3, sg, 3, T, loaded=True, streamed_side=True, max_records=64)
                assert e.last_path() == path, (path, m)
                check(got, reference(m, truths[m], T, lg, 3, sg, 3), (path, m))
                results[path, m] = got
        for m in ("raw", "tn93"):
            for k in CELL_KEYS + REC_KEYS:
                assert np.array_equal(bits(results["dense", m][0][k]), bits(results["consensus", m][0][k])), (m, k)


# ---- 8. one group on each side is the summary stream -----------------------------------------------------------------------------
@pytest.mark.parametrize("measure", ["n", "raw", "tn93"])
def test_one_group_each_side_is_the_summary_stream(eng, data, measure):
    loaded, streamed = data[0][:COLS + 1], data[1]
    eng.upload(0, loaded)
    T = median_of(truth(eng, COLS + 1, measure, streamed))
    got = run_groups(eng, measure, streamed, cuts_of(N_S, MAXREC), None, 1, None, 1, T, loaded=True, streamed_side=True)
    sides = []
    with eng.summary_stream(measure, MAXREC, threshold=T, loaded=True, streamed=True) as st:
        for b0 in range(0, N_S, MAXREC):
            st.push(streamed[b0:b0 + MAXREC])
            sides.append(st.pop())
        plain = st.result()
    res = got[0]
    for key, mine in (("pairs", "pairs"), ("nan_pairs", "nan_pairs"), ("summable_pairs", "summable_pairs"), ("links", "links")):
        assert int(res[mine][0, 0]) == plain[key], key
    assert bits(res["sum"])[0, 0] == bits(np.float64(plain["total_sum"]))
    for a, (mine, key) in enumerate((("rec_within", "within"), ("rec_summable", "summable"), ("rec_sum", "sum"))):
        assert np.array_equal(bits(res[mine][:, 0]), bits(plain[key])), key
        assert np.array_equal(bits(got[1][a][:, 0]), bits(np.concatenate([s[a + 1] for s in sides]))), key


# ---- 9. the whole stream uploaded to slot 1 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", ["n", "jc69", "tn93"])
def test_the_stream_as_a_loaded_set(data, measure):
    loaded, streamed = data[0][:COLS + 1], data[1]
    lg, sg = labels(COLS + 1, 3, "random", 11), labels(N_S, 5, "random", 12)
    with da.Engine(0) as e:
        e.upload(0, loaded)
        e.upload(1, streamed)
        T = median_of(e.run_rect(measure, row_slot=1, col_slot=0))
        want = e.group_summary(measure, sg, 5, threshold=T, square=False, row_slot=1, col_slot=0, col_groups=lg, n_col_groups=3,
                               per_record=True)
        got = run_groups(e, measure, streamed, cuts_of(N_S, MAXREC), lg, 3, sg, 5, T, streamed_side=True)
        for k in CELL_KEYS:
            assert np.array_equal(bits(got[0][k]), bits(want[k])), (measure, k)
        for a, k in enumerate(REC_KEYS):
            assert np.array_equal(bits(got[1][a]), bits(want[k])), (measure, k)
        check_consequences(dict(got[0], rec_within=got[1][0], rec_summable=got[1][1], rec_sum=got[1][2]), sg, False)


# ---- 10. snapshots, and other calls on the context in between --------------------------------------------------------------------
def test_snapshots_and_other_calls_in_between(data):
    loaded, streamed = data[0][:COLS + 1], data[1]
    lg, sg = labels(COLS + 1, 3, "random", 13), labels(N_S, 3, "random", 14)
    with da.Engine(0) as e:
        e.upload(0, loaded)
        S = plain_truth(e, "k80", streamed, max_records=MAXREC)[0]
        T = median_of(S)
        groups_before = e.group_summary("k80", lg, 3, threshold=T, per_record=True)
        summary_before = e.summary("k80", threshold=T, bins=8, width=0.05)
        square_before = e.run_square("k80")
        with e.group_summary_stream("k80", 16, loaded_groups=lg, n_loaded_groups=3, n_streamed_groups=3, threshold=T,
                                    loaded=True, streamed=True) as st:
            empty = st.result()
            assert empty["records"] == 0 and not empty["pairs"].any() and not empty["rec_summable"].any()
            check_empty_rules("k80", empty)
            for b0 in range(0, 64, 16):
                st.push(streamed[b0:b0 + 16], groups=sg[b0:b0 + 16])
                # the context's own group summary (its group buffers), summary and square between a submit and its collect
                assert_group_summary(e.group_summary("k80", lg, 3, threshold=T, per_record=True), groups_before, "in between")
                assert_summary(e.summary("k80", threshold=T, bins=8, width=0.05), summary_before, "dst_summary in between")
                assert np.array_equal(bits(e.run_square("k80")), bits(square_before))
                side = st.pop()
                want = reference("k80", S[:b0 + 16], T, lg, 3, sg[:b0 + 16], 3)
                check((st.result(), None), want, ("snapshot", b0))
                check((st.result(), None), want, ("snapshot again", b0))
                assert all(np.array_equal(bits(a), bits(b[b0:b0 + 16])) for a, b in zip(side[1:], want[1])), b0
        assert_group_summary(e.group_summary("k80", lg, 3, threshold=T, per_record=True), groups_before, "afterwards")


# ---- 11. an invalid code ------------------------------------------------------------------------------------------------------------
def test_an_invalid_code_poisons_the_stream(eng, data):
    loaded, streamed = data[0][:COLS + 1], data[1]
    eng.upload(0, loaded)
    S = truth(eng, COLS + 1, "raw", streamed)
    lg, sg = labels(COLS + 1, 3, "random", 15), labels(N_S, 3, "random", 16)
    with eng.group_summary_stream("raw", 8, loaded_groups=lg, n_streamed_groups=3, n_loaded_groups=3, loaded=True, streamed=True) as st:
        st.push(streamed[:8], groups=sg[:8])
        buf, _ = st.buffer()
        bad = streamed[8:12].copy()
        bad[2, 60] = 7
        buf[:4] = bad
        st.submit(4)
        assert st.pop()[0] == 8
        with pytest.raises(da.DistanceError) as e:
            st.pop()
        assert e.value.status == ERR_INVALID_CODE and "record 2 at site 6" in e.value.message
        assert status_of(st.group_summary_batch) == ERR_STATE
        assert status_of(st.result) == ERR_STATE
        assert status_of(st.push, streamed[12:20]) == ERR_STATE  # the batch's atomics cannot be taken back
        assert status_of(st.result) == ERR_STATE
    # close worked; a fresh stream on the same context gives the right answer
    check(run_groups(eng, "raw", streamed, cuts_of(N_S, MAXREC), lg, 3, sg, 3, 0.05, loaded=True, streamed_side=True),
          reference("raw", S, 0.05, lg, 3, sg, 3), "fresh")


# ---- 12. misuse: the documented statuses -------------------------------------------------------------------------------------------
def test_open_errors_in_the_documented_order(eng, data):
    lib = da.load()
    eng.upload(0, data[0][:130])
    h = C.c_void_p()
    good = labels(130, 3, "interleaved")

    def open_(ctx, measure=2, T=1.0, what=3, lg=good, Gl=3, Gs=2, max_records=8, depth=3, wire=0, out=C.byref(h)):
        return lib.dst_stream_open_group_summary(ctx, measure, T, what, None if lg is None else lg.ctypes.data, Gl, Gs, max_records,
                                                 depth, wire, out)

    assert open_(None) == ERR_ARG and open_(eng._h, out=None) == ERR_ARG
    for bad in (dict(measure=9), dict(measure=-1), dict(wire=2), dict(T=float("nan")), dict(what=4), dict(what=-1), dict(Gl=0),
                dict(Gs=0), dict(Gl=1025), dict(Gs=1025), dict(lg=None, Gl=2), dict(max_records=0), dict(depth=1), dict(depth=17)):
        assert open_(eng._h, **bad) == ERR_ARG, bad
        assert h.value is None
    wrong = good.copy()
    wrong[77] = 3
    assert open_(eng._h, lg=wrong) == ERR_ARG
    message = lib.dst_last_error(eng._h).decode()
    assert "record 77 has label 3" in message and "loaded" in message
    assert open_(eng._h, lg=None, Gl=1) == 0
    lib.dst_stream_close(h)
    with da.Engine(0) as fresh:                                            # slot 0 not loaded: behind every argument error
        assert status_of(fresh.group_summary_stream, "raw", 8) == ERR_STATE
        assert open_(fresh._h, what=4) == ERR_ARG and open_(fresh._h, depth=1) == ERR_ARG and open_(fresh._h, Gs=1025) == ERR_ARG
        assert open_(fresh._h, lg=wrong) == ERR_STATE


def test_misuse(eng, data):
    lib = da.load()
    loaded, streamed = data[0][:130], data[1]
    eng.upload(0, loaded)
    lg = labels(130, 3, "interleaved")
    n, wp, sp, dp, ku, lp = C.c_size_t(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint32(), C.c_void_p()
    total, late = C.c_uint64(), C.c_uint64()
    every = (C.byref(n), C.byref(wp), C.byref(sp), C.byref(dp))
    room = np.zeros(130 * 2, np.uint32)
    sums = np.zeros(130 * 2, np.float64)
    cells = (da._lib.GroupCell * 6)()

    def result(st, cells=None, cells_cap=6, within=None, summable=None, sum_=None, cap=260):
        return lib.dst_stream_group_summary_result(st._h, cells, cells_cap, within, summable, sum_, cap, None)

    with eng.group_summary_stream("raw", 8, loaded_groups=lg, n_loaded_groups=3, n_streamed_groups=2, threshold=0.05,
                                  loaded=True, streamed=True) as st:
        assert lib.dst_stream_group_summary_batch(st._h, *every) == ERR_STATE        # no collected batch
        assert lib.dst_stream_group_labels(st._h, C.byref(lp)) == ERR_STATE          # no buffer acquired
        buf, _ = st.buffer()
        assert lib.dst_stream_group_labels(st._h, None) == ERR_ARG
        block = st.labels()
        assert block.shape == (8,) and not block.any()                                # filled with 0 by the acquire
        block[:8] = [0, 1, 0, 1, 2, 0, 1, NONE]                                       # 2 is neither below the count nor NONE
        buf[:8] = streamed[:8]
        assert status_of(st.submit, 8) == ERR_ARG
        assert "record 4 has label 2" in lib.dst_last_error(eng._h).decode()
        assert st.in_flight() == 0 and result(st) == 0                                # ... and changed nothing
        block[4] = 1
        st.submit(8)
        assert lib.dst_stream_group_labels(st._h, C.byref(lp)) == ERR_STATE
        assert lib.dst_stream_group_summary_batch(st._h, *every) == ERR_STATE
        assert status_of(st.result) == ERR_STATE                                     # a batch in flight
        assert st.pop()[0] == 8
        assert st.result()["records"] == 8 and int(st.result()["pairs"].sum()) == 7 * 130
        assert lib.dst_stream_group_summary_batch(st._h, None, *every[1:]) == ERR_ARG
        assert lib.dst_stream_group_summary_batch(st._h, C.byref(n), None, None, None) == 0 and n.value == 8
        assert result(st, cells=C.addressof(cells), cells_cap=5) == ERR_CAPACITY
        assert result(st, within=room.ctypes.data, cap=259) == ERR_CAPACITY          # below n_loaded x G_s
        assert result(st, sum_=sums.ctypes.data, cap=0) == ERR_CAPACITY
        assert result(st, cells=C.addressof(cells), cells_cap=6, cap=0) == 0          # no per-record array: cap is not read
        assert result(st, within=room.ctypes.data, summable=room.ctypes.data, sum_=sums.ctypes.data, cells_cap=0) == 0
        # the other kinds' calls on this stream
        index = np.zeros(1040, np.uint32)
        assert lib.dst_stream_closest_batch(st._h, C.byref(sp), C.byref(wp), C.byref(dp), C.byref(ku)) == ERR_ARG
        assert lib.dst_stream_closest_result(st._h, index.ctypes.data, None, None, 1040, C.byref(ku)) == ERR_ARG
        assert lib.dst_stream_closest_next_index(st._h, 5) == ERR_ARG
        assert lib.dst_stream_links_batch(st._h, 0, C.byref(total), C.byref(late), C.byref(sp), C.byref(wp), None, None) == ERR_ARG
        assert lib.dst_stream_links_stats(st._h, C.byref(total), C.byref(late)) == ERR_ARG
        assert lib.dst_stream_window_closest_result(st._h, index.ctypes.data, None, None, None, 1040, C.byref(ku)) == ERR_ARG
        assert lib.dst_stream_summary_batch(st._h, *every) == ERR_ARG
        assert lib.dst_stream_summary_result(st._h, None, None, None, None, 0, None, None) == ERR_ARG
        eng.upload(0, loaded[:100])                                                  # the loaded set's record count changed
        assert status_of(st.push, streamed[:8]) == ERR_STATE
    eng.upload(0, loaded)
    with eng.group_summary_stream("raw", 8, streamed=True) as st:                    # a table that was not asked for
        st.push(streamed[:8])
        st.pop()
        for kw in (dict(within=room.ctypes.data), dict(summable=room.ctypes.data), dict(sum_=sums.ctypes.data)):
            assert result(st, **kw) == ERR_ARG, kw
        assert result(st) == 0
    with eng.group_summary_stream("raw", 8, loaded=True) as st:                      # ... and the other one
        st.push(streamed[:8])
        assert st.pop() == 8
        assert lib.dst_stream_group_summary_batch(st._h, *every) == ERR_ARG
    # this kind's calls on the other kinds, and on no stream at all
    for other in (eng.stream("raw", max_records=8, depth=2), eng.closest_stream("raw", 5, 8),
                  eng.closest_stream("raw", 5, 8, side="streamed"), eng.links_stream("raw", 0.05, 8),
                  eng.window_closest_stream("raw", [(0, 48), (48, 96)], 2, 8), eng.summary_stream("raw", 8)):
        with other as st:
            st.buffer()
            assert lib.dst_stream_group_labels(st._h, C.byref(lp)) == ERR_ARG
            assert lib.dst_stream_group_summary_batch(st._h, *every) == ERR_ARG
            assert result(st) == ERR_ARG
    assert lib.dst_stream_group_labels(None, C.byref(lp)) == ERR_ARG
    assert lib.dst_stream_group_summary_batch(None, *every) == ERR_ARG
    assert lib.dst_stream_group_summary_result(None, None, 0, None, None, None, 0, None) == ERR_ARG


def test_a_plain_stream_afterwards(data):
    """(An empty loaded set cannot arise: dst_upload refuses n = 0.)"""
    loaded, streamed = data[0][:130], data[1]
    lg, sg = labels(130, 2, "random", 17), labels(N_S, 2, "random", 18)
    with da.Engine(0) as e:
        e.upload(0, loaded)
        before = plain_truth(e, "tn93", streamed, max_records=MAXREC)
        check(run_groups(e, "tn93", streamed, cuts_of(N_S, MAXREC), lg, 2, sg, 2, 0.05, loaded=True, streamed_side=True),
              reference("tn93", before[0], 0.05, lg, 2, sg, 2), "tn93")
        after = plain_truth(e, "tn93", streamed, max_records=MAXREC)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(after, before))   # a plain stream still delivers its matrix
