"""GPU (-m gpu): the streaming form of the pack (pack_stream_kernel) — what an upload for the consensus
path runs on the whole 1 KiB spans of its rows: rows read as streams and compared with the reference sequence's bytes,
and only the (record, chunk)s with something in them handed to the per-chunk code every other upload runs.  It must leave
exactly what pack_kernel leaves (slots, counters, run counters, the first invalid byte, the planes of the chunks that do
not fit their slot), so every case here uploads a low-diversity set with the deferring form (asserted), runs all six
measures on the consensus path against an engine that packs every plane and runs dense (bit for bit), samples the oracle,
and reads the base counts (from the slots) and the differences (from the planes written back from the slots).
Shapes sit on the kernel's boundaries: a block is R = 64 records x 8 chunks, a wave 16 of the records."""
import numpy as np
import pytest

import distance_amd as da
import oracle

pytestmark = pytest.mark.gpu
ALL = ("n", "n_high", "raw", "jc69", "k80", "tn93")
BASES = np.array([136, 72, 40, 24], np.uint8)
NEXT = {136: 72, 72: 40, 40: 24, 24: 136}
R = 64   # kStreamRows


@pytest.fixture(scope="module")
def engines():
    with da.Engine(0) as ref, da.Engine(0) as eng:
        ref.set_path("dense")
        eng.set_prep_threshold(0)
        yield ref, eng


def low_diversity_set(n, L, seed, rate=0.002):
    rng = np.random.default_rng([seed, n, L])
    root = rng.choice(BASES, size=L)
    codes = np.tile(root, (n, 1))
    mut = rng.random((n, L)) < rate
    codes[mut] = rng.choice(BASES, size=int(mut.sum()))
    return codes, root


def substitute(codes, root, r, sites):
    for s in sites:
        codes[r, s] = NEXT[int(root[s])]


def check(engines, codes, path="consensus", upload=None, oracle_pairs=8, oracle_consensus=True):
    """every measure on `path` after a deferring upload == dense after a full pack; the oracle on sampled pairs; counts;
    differences"""
    ref, eng = engines
    n, L = codes.shape
    flat = np.ascontiguousarray(codes)
    ref.set_path("dense")
    ref.upload(0, flat)
    assert ref.planes_stored(0)
    want = {m: ref.run_square(m) for m in ALL}
    eng.set_path("auto")
    if upload is None:
        eng.upload(0, codes)
    else:
        upload(eng)
    assert not eng.planes_stored(0), "the upload stored every plane: the deferring form did not run"
    eng.set_path(path)
    got = {}
    for m in ALL:
        got[m] = eng.run_square(m)
        assert eng.last_path() == path, (m, eng.last_path())
        assert np.array_equal(got[m], want[m], equal_nan=True), m
    rng = np.random.default_rng(n * 1_000_003 + L)
    for _ in range(oracle_pairs):
        i = int(rng.integers(0, n - 1))
        j = int(rng.integers(i + 1, n))
        at = da.square_row_start(n, i) + j - i - 1
        for m in ("n_high", "raw", "tn93"):
            w = oracle.pair_distance(m, flat[i], flat[j])
            if m == "n_high":
                assert int(got[m][at]) == int(w), (m, i, j)
            else:
                assert np.isclose(got[m][at], w, rtol=0, atol=1e-12, equal_nan=True), (m, i, j)
    rows = sorted(set(range(min(n, 12))) | {n // 2, n - 1})
    counts = eng.base_counts(0)
    assert np.array_equal(counts[rows], np.stack([oracle.count_bases(flat[r]) for r in rows]))
    cons = eng.consensus()
    if oracle_consensus:
        assert np.array_equal(cons, oracle.consensus(flat))
    diffs = eng.differences(0, cons)
    for r in rows:
        assert np.array_equal(diffs[r].astype(np.uint64), oracle.get_differences(flat[r], cons)), r
    return got


# ---- records x widths at the block's edges -----------------------------------------------------------------------
@pytest.mark.parametrize("L", [1024, 1040, 2048 + 48, 128 * 9, 1024 * 3 - 16])
@pytest.mark.parametrize("n", [2, R - 1, R, R + 1, 2 * R + 1, 300])
def test_records_and_widths_at_the_block_edges(engines, n, L):
    codes, root = low_diversity_set(n, L, 1)
    substitute(codes, root, n - 1, [0, L - 1])                 # the set's corners
    substitute(codes, root, 0, [1023, min(1024, L - 1)])       # the last site of a span, the first behind it
    check(engines, codes)


# ---- a slot holds 7: 7 and 8 differences in one chunk, in one lane's 16 sites and one per lane ---------------------------
def test_seven_and_eight_differences_in_one_lane_and_spread(engines):
    n, L = 70, 2048
    codes, root = low_diversity_set(n, L, 2, rate=0.0)
    c2, c3, c9 = 2 * 128, 3 * 128, 9 * 128
    substitute(codes, root, 5, [c2 + 48 + k for k in range(7)])          # 7 in lane 3 of the chunk
    substitute(codes, root, 6, [c2 + 48 + k for k in range(8)])          # 8 in that lane
    substitute(codes, root, 7, [c3 + 16 * k for k in range(7)])          # 7, one per lane
    substitute(codes, root, 8, [c3 + 16 * k + k for k in range(8)])      # 8, one per lane
    substitute(codes, root, 9, [c9 + 15, c9 + 16])                       # two lanes of one chunk
    substitute(codes, root, 10, [c9 + 127, c9 + 128])                    # two chunks
    substitute(codes, root, 64, [c2 + 48 + k for k in range(7)] + [c3 + 16 * k + k for k in range(8)])   # the next block
    got = check(engines, codes)
    assert int(got["n_high"][da.square_row_start(n, 5) + 1]) == 7 + 7    # records 5 and 7 share none


# ---- one lane position differs in R consecutive records: every bit of the lane's masks, a full queue for the chunk -------
@pytest.mark.parametrize("first", [0, R, R - 5])
def test_one_lane_differs_in_every_record_of_a_block(engines, first):
    n, L = 3 * R + 8, 2048
    codes, root = low_diversity_set(n, L, 3, rate=0.0005)
    for r in range(first, first + R):
        substitute(codes, root, r, [1024 + 16 * 5 + 3])
    check(engines, codes)


# ---- chunks of N (N, -) over a known reference, and a record that is nothing but N ------------------------------------
def test_run_chunks_and_a_record_of_n(engines):
    n, L = 80, 2048 + 48
    codes, root = low_diversity_set(n, L, 4)
    codes[3, 128 * 2:128 * 5] = 240
    codes[4, 128 * 7:128 * 10] = 244        # across the span's edge
    codes[5, 128 * 13:128 * 16 + 48] = 240  # the last whole span's end and the tail chunk
    codes[70, :] = 240
    codes[71, 100:700] = 242                # partial chunks at both ends
    check(engines, codes)


# ---- a difference in the low nibble only (- and ? where the reference is N) is no difference ---------------------------
def test_low_nibble_only_differences_add_nothing(engines):
    n, L = 90, 2048
    codes, root = low_diversity_set(n, L, 5)
    codes[:, 300:340] = 240
    codes[:, 1500:1510] = 240
    plain = codes.copy()
    codes[7, 300:320] = 244
    codes[8, 310:335] = 242
    codes[66, 1500:1510] = 244
    _, eng = engines
    a = check(engines, plain)
    length_plain = eng.last_launch()["list_length"]
    b = check(engines, codes)
    assert eng.last_launch()["list_length"] == length_plain
    for m in ALL:
        assert np.array_equal(a[m], b[m], equal_nan=True), m


# ---- hot sites: a third of the records share substitutions at 2 % of the sites -----------------------------------------
def test_clade_sites_on_the_hybrid_path(engines):
    n, L = 200, 3072
    codes, root = low_diversity_set(n, L, 6)
    rng = np.random.default_rng(6)
    sites = np.sort(rng.choice(L, L // 50, replace=False))
    for r in rng.choice(n, n // 3, replace=False):
        substitute(codes, root, int(r), sites)
    check(engines, codes, path="hybrid")
    check(engines, codes, path="consensus")


# ---- invalid bytes ----------------------------------------------------------------------------------------------
def expect_invalid(eng, codes, record, site):
    with pytest.raises(da.DistanceError) as e:
        eng.upload(0, codes)
    assert f"record {record} at site {site} " in str(e.value), str(e.value)


def test_invalid_bytes_are_named_exactly(engines):
    _, eng = engines
    n, L = 150, 2048 + 48
    codes, root = low_diversity_set(n, L, 7)
    eng.set_path("auto")
    # the reference's high nibble with a low nibble no code has
    bad = codes.copy()
    bad[20, 777] = (int(root[777]) & 0xF0) | 9
    expect_invalid(eng, bad, 20, 777)
    # 0x00 in a streamed span, and in the tail chunk
    bad = codes.copy()
    bad[100, 1500] = 0
    expect_invalid(eng, bad, 100, 1500)
    bad = codes.copy()
    bad[100, 2048 + 40] = 0
    expect_invalid(eng, bad, 100, 2048 + 40)
    # two of them in different blocks: the earlier one by (record, site), whichever block finishes first
    bad = codes.copy()
    bad[130, 5] = 0
    bad[30, 2000] = 1
    expect_invalid(eng, bad, 30, 2000)
    bad = codes.copy()
    bad[30, 1030] = 0x89
    bad[30, 1000] = 0xF1
    expect_invalid(eng, bad, 30, 1000)
    # in a chunk that also has more differences than its slot holds
    bad = codes.copy()
    substitute(bad, root, 40, [128 * 4 + 3 * k for k in range(20)])
    bad[40, 128 * 4 + 100] = 0x0F
    expect_invalid(eng, bad, 40, 128 * 4 + 100)
    # and the engine is fine afterwards
    check(engines, codes)


# ---- what the streaming form does not take still goes the old way ------------------------------------------------------
def test_odd_width_and_strided_views(engines):
    torch = pytest.importorskip("torch")
    n = 150
    codes, root = low_diversity_set(n, 1039, 8)
    codes[9, 128 * 3:128 * 5] = 240
    check(engines, codes)                                  # one streamed span and a partial tail chunk
    wide, _ = low_diversity_set(n, 1039 + 1024 + 21, 8)
    view = wide[:, 5:5 + 1040]                             # a view: row stride 2084, no multiple of 16
    assert not view.flags["C_CONTIGUOUS"] and view.strides[0] % 16
    check(engines, view)
    # rows off 16-byte boundaries on the device: pack_kernel's shifted path for every chunk
    dwide = torch.from_numpy(wide).cuda()
    dview = dwide[:, 5:5 + 1040]
    check(engines, view, upload=lambda e: e.upload_device(0, dview.data_ptr(), n, 1040, dview.stride(0)))
    torch.cuda.synchronize()


# ---- the shared upload: each rank streams its own records.  (dst_shared_range cuts at multiples of 256 records, so a
# rank's range starts on a block's edge; the only range that ends inside a block's R rows is the one that ends the set.)
def test_shared_upload_streams_each_rank_s_records():
    torch = pytest.importorskip("torch")
    from shared_ranks import ThreadRanks, single_engine
    n, L, world = 300, 2048 + 48, 2
    cut = da.shared_range(n, 0, world)[1]
    assert 0 < cut < n and da.shared_range(n, 1, world) == (cut, n) and (n - cut) % R
    codes, root = low_diversity_set(n, L, 9)
    codes[cut - 1, 128:128 * 4] = 240
    substitute(codes, root, cut, [128 * 5 + k for k in range(9)])
    dcodes = torch.from_numpy(codes).cuda()
    want = single_engine(codes, ALL)
    bounds = da.partition_square(n, world)

    def body(rank, eng, comm):
        eng.set_prep_threshold(0)
        eng.upload_shared(comm, 0, dcodes.data_ptr(), n, L, dcodes.stride(0), with_counts=True)
        st = eng.shared_stats()
        assert st["shared_uploads"] == 1 and st["fallbacks"] == 0, st
        assert not eng.planes_stored(0), "the shared upload stored planes: the deferring form did not run"
        got = {}
        for m in ALL:
            got[m] = eng.run_square(m, bounds[rank], bounds[rank + 1])
            assert eng.last_path() == "consensus", m
        assert not eng.planes_stored(0)
        got["counts"] = eng.base_counts(0)
        return got

    res = ThreadRanks(world).run(body)
    counts = np.stack([oracle.count_bases(r) for r in codes])
    rng = np.random.default_rng(9)
    for rank in range(world):
        lo, hi = da.square_row_start(n, bounds[rank]), da.square_row_start(n, bounds[rank + 1])
        for m in ALL:
            assert np.array_equal(res[rank][m], want[m][lo:hi], equal_nan=True), (rank, m)
        assert np.array_equal(res[rank]["counts"], counts), rank
        # the oracle on pairs of this rank's rows, the records on either side of the cut among the columns
        for j in (cut - 1, cut, n - 1, None, None, None, None):
            i = int(rng.integers(bounds[rank], min(bounds[rank + 1], cut - 1)))
            j = int(rng.integers(i + 1, n)) if j is None else j
            at = da.square_row_start(n, i) + j - i - 1 - lo
            assert int(res[rank]["n_high"][at]) == int(oracle.pair_distance("n_high", codes[i], codes[j])), (rank, i, j)
            for m in ("raw", "tn93"):
                assert np.isclose(res[rank][m][at], oracle.pair_distance(m, codes[i], codes[j]), rtol=0, atol=1e-12,
                                  equal_nan=True), (rank, m, i, j)


# ---- fuzz ---------------------------------------------------------------------------------------------------------
IUPAC = np.array([192, 160, 144, 96, 80, 48, 224, 176, 208, 112, 244, 242], np.uint8)


@pytest.mark.parametrize("seed", range(40))
def test_fuzz_equals_dense(engines, seed):
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(2, 301))
    # (widths of 16 x (64 .. 200) reach the streaming kernel; every fifth set is narrower and goes the old way whole)
    L = 16 * int(rng.integers(1, 64) if seed % 5 == 4 else rng.integers(64, 201))
    rate = (0.001, 0.01, 0.05)[int(rng.integers(0, 3))]
    codes, root = low_diversity_set(n, L, 100 + seed, rate=rate)
    for _ in range(int(rng.integers(0, 4))):                     # runs of N: some span chunks, some do not
        r, a = int(rng.integers(0, n)), int(rng.integers(0, L))
        w = int(rng.integers(1, 400)) if n >= 20 else int(rng.integers(1, L // 32 + 2))   # (a small set stays low-diversity)
        codes[r, a:a + w] = 240
    amb = rng.random((n, L)) < 0.003
    codes[amb] = rng.choice(IUPAC, size=int(amb.sum()))
    # (the consensus call's own ties on sets of a few records are not this file's subject: differences are still checked
    # against the oracle, with the consensus the engine returned)
    check(engines, codes, oracle_pairs=4, oracle_consensus=False)
    ref, eng = engines
    assert np.array_equal(eng.base_counts(0), ref.base_counts(0))
