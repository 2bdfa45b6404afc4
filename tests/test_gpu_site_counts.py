"""GPU (-m gpu): dst_site_counts against site_counts_reference (numpy on the code matrix), bitwise: the record and site
shapes around a wave, a strip and a chunk, every kind of labelling, site ranges inside a chunk, every code in every column
position, counts past every counter width the kernel could have, stale padding, a deferring upload, the state the call
must leave alone, and every documented error.  Shapes are the smallest at which the kernel can go wrong."""
import ctypes as C

import numpy as np
import pytest

import distance_amd as da
from distance_amd import _lib
from helpers import CODES, random_alignment, uniform_codes
from site_counts_reference import CLASSES, NONE, site_counts
from tools import synth

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE, ERR_CAPACITY = 1, 4, 6
STRIP, PERIOD = _lib.SITE_STRIP_RECORDS, _lib.SITE_FLUSH_PERIOD
A, G, T, N, R = 136, 72, 24, 240, 192


@pytest.fixture(scope="module")
def eng():
    with da.Engine(0) as e:
        yield e


def check(eng, codes, groups=None, n_groups=None, begin=0, end=None):
    got = eng.site_counts(0, groups, n_groups, begin, end)
    G_ = 1 if groups is None else (n_groups if n_groups is not None else int(np.max(groups)) + 1)
    want = site_counts(codes, groups, G_, begin, end)
    assert got.dtype == np.uint32 and got.shape == want.shape
    assert np.array_equal(got, want), (codes.shape, G_, begin, end, np.argwhere(got != want)[:5].tolist())
    return got


@pytest.mark.parametrize("n", [1, 63, 64, 65, STRIP - 1, STRIP, STRIP + 1])
def test_record_and_site_shapes(eng, n):
    for length in (1, 127, 128, 129, 257):
        codes = uniform_codes(n, length, 1000 * n + length)
        eng.upload(0, codes)
        check(eng, codes)
        if n >= 63:   # two groups interleaved with unassigned records: strips that end inside a wave
            check(eng, codes, np.arange(n) % 3 - 1, 2)


LABELLINGS = {
    "2 contiguous": lambda n: (np.arange(n) >= n // 3).astype(np.int64),
    "3 contiguous": lambda n: np.minimum(np.arange(n) * 3 // n, 2),
    "2 interleaved": lambda n: np.arange(n) % 2,
    "3 interleaved": lambda n: np.arange(n) % 3,
    "unassigned records": lambda n: np.where(np.arange(n) % 5 == 0, -1, np.arange(n) % 3),
    "random": lambda n: np.random.default_rng(n).integers(-1, 4, n),
}


@pytest.mark.parametrize("name", list(LABELLINGS))
def test_group_labellings(eng, name):
    n, length = STRIP + 700, 300    # every group of the contiguous cases and group 0 of the interleaved pair pass no strip edge,
    codes = random_alignment(n, length, 21, p_ambig=0.1, p_gap=0.1, divergence=0.3)   # the contiguous pair's second group does
    eng.upload(0, codes)
    g = LABELLINGS[name](n)
    check(eng, codes, g, int(g.max()) + 1)


def test_empty_group_all_unassigned_and_most_groups(eng):
    n, length = 1030, 200
    codes = uniform_codes(n, length, 5)
    eng.upload(0, codes)
    g = np.array([0, 2, 3])[np.arange(n) % 3]
    got = check(eng, codes, g, 5)                       # groups 1 and 4 are empty
    assert not got[:, 1].any() and not got[:, 4].any()
    assert not eng.site_counts(0, np.full(n, -1), 3).any()   # nobody assigned: zeros, no launch
    check(eng, codes, np.arange(n) % 1024, 1024)          # DST_GROUPS_MAX groups, six of them of two records
    check(eng, codes, np.where(np.arange(n) % 2 == 1, NONE, 0), 1)   # 2^32-1 as "no group"


def test_site_ranges_inside_a_chunk(eng):
    n, length = 130, 700
    codes = uniform_codes(n, length, 9)
    eng.upload(0, codes)
    g = np.arange(n) % 2
    for begin, end in [(0, 0), (5, 5), (700, 700), (0, 1), (3, 30), (31, 33), (100, 128), (100, 129), (127, 257), (128, 256),
                       (130, 250), (640, 700), (699, 700), (1, 699)]:
        check(eng, codes, None, None, begin, end)
        check(eng, codes, g, 2, begin, end)


def test_every_code_in_every_column_position(eng):
    """17 records per block of 17 rotations: column c of record r holds code (r + c) % 17, so every column position of a
    chunk meets every code, and every class count is known without the reference too"""
    length = 2 * 128 + 17
    n = 17 * 4
    codes = CODES[(np.arange(n)[:, None] + np.arange(length)[None, :]) % 17]
    eng.upload(0, codes)
    got = check(eng, codes)
    assert (got[:, 0, :4] == 4).all() and (got[:, 0, 4] == 40).all()   # 4 of each base, 10 ambiguity codes x 4, 3 x 4 missing
    check(eng, codes, np.arange(n) // 17, 4)


def test_counter_saturation(eng):
    n, length = 70_000, 256
    codes = np.full((n, length), A, np.uint8)
    codes[:, 1::4] = N
    codes[:, 2::4] = R
    codes[0::2, 3::4], codes[1::2, 3::4] = G, T
    eng.upload(0, codes)
    for groups, sizes in ((None, [n]), ((np.arange(n) >= n // 2).astype(np.int64), [n // 2, n // 2])):
        got = eng.site_counts(0, groups)
        for g, size in enumerate(sizes):
            z = np.zeros(5, np.uint32)
            want = np.stack([np.array([size, 0, 0, 0, 0]), z, np.array([0, 0, 0, 0, size]), np.array([0, size // 2, size // 2, 0, 0])])
            assert np.array_equal(got[:, g], np.tile(want, (length // 4, 1))), (g, got[:8, g].tolist())


def test_stale_padding_is_not_counted(eng):
    eng.upload(0, np.full((900, 400), A, np.uint8))   # the slot's buffers are kept: whatever the next pack leaves behind
    codes = uniform_codes(65, 129, 3)
    eng.upload(0, codes)
    check(eng, codes)
    check(eng, codes, np.arange(65) % 2, 2)


def test_after_a_deferring_upload():
    n, length = 2_000, 5_000
    codes = synth.alignment(synth.SEED ^ 77, n, length)
    codes[7, 100:400] = N
    codes[9, ::37] = R
    g = np.arange(n) % 3
    with da.Engine(0) as e:
        e.set_prep_threshold(0)
        e.upload(0, codes)
        assert not e.planes_stored(0), "the upload stored every plane: nothing here tests the deferred form"
        check(e, codes, g, 3)
        assert e.planes_stored(0)
        check(e, codes)


def test_leaves_runs_and_the_path_alone(eng):
    codes = random_alignment(300, 900, 4)
    eng.upload(0, codes)
    for path in ("dense", "consensus"):
        eng.set_path(path)
        before = {m: eng.run_square(m) for m in ("n", "raw", "tn93")}
        assert eng.last_path() == path
        launch = eng.last_launch()
        check(eng, codes, np.arange(300) % 4, 4)
        assert eng.last_path() == path and eng.last_launch() == launch
        for m, want in before.items():
            assert np.array_equal(eng.run_square(m).view(np.uint64), want.view(np.uint64)), (path, m)
    eng.set_path("auto")


def test_shared_set_is_refused():
    from shared_ranks import ThreadRanks
    from test_gpu_windows import Hip
    n, length = 2_500, 3_000
    codes = synth.alignment(synth.SEED ^ 9, n, length)
    hip = Hip()
    d_codes = hip.to_device(codes)

    def body(rank, e, comm):
        e.upload_shared(comm, 0, d_codes, n, length, length, with_counts=True)
        assert e.shared_stats()["fallbacks"] == 0
        with pytest.raises(da.DistanceError) as err:
            e.site_counts(0)
        return err.value.status, err.value.message

    try:
        for status, message in ThreadRanks(2).run(body):
            assert status == ERR_STATE and "dst_upload_shared runs on the consensus path only" in message
    finally:
        hip.lib.hipFree(d_codes)


def test_errors_in_their_order():
    lib = da.load()
    n, length = 9, 90
    codes = uniform_codes(n, length, 2)
    out = np.full(length * 2 * CLASSES + 8, 7, np.uint32)
    g = (np.arange(n) % 2).astype(np.uint32)
    with da.Engine(0) as e:
        h = e._h

        def call(slot=0, group=g, G=2, begin=0, end=length, counts=out, cap=None):
            return lib.dst_site_counts(h, slot, None if group is None else group.ctypes.data, G, begin, end,
                                       None if counts is None else counts.ctypes.data, out.size if cap is None else cap)

        def message():
            return lib.dst_last_error(h).decode()

        assert lib.dst_site_counts(None, 0, None, 1, 0, 0, out.ctypes.data, out.size) == ERR_ARG
        # the first tier comes before the set's state: nothing is uploaded yet
        assert call(counts=None) == ERR_ARG and call(slot=2) == ERR_ARG and call(slot=-1) == ERR_ARG
        assert call(G=0) == ERR_ARG and call(G=_lib.GROUPS_MAX + 1) == ERR_ARG and "between 1 and 1024" in message()
        assert call(group=None, G=2) == ERR_ARG
        assert call() == ERR_STATE and "not uploaded" in message()
        e.upload(0, codes)
        assert call(slot=1) == ERR_STATE
        assert call(begin=5, end=4) == ERR_ARG and call(end=length + 1) == ERR_ARG and "[0, 91)" in message()
        bad = g.copy()
        bad[4], bad[6] = 2, 9
        assert call(group=bad) == ERR_ARG
        assert "record 4 has label 2, which is neither below the group count 2 nor DST_GROUP_NONE" in message()
        # a bad label comes before the capacity, a bad range before a bad label
        assert call(group=bad, cap=0) == ERR_ARG and call(group=bad, end=length + 1) == ERR_ARG and "[0, 91)" in message()
        assert call(cap=length * 2 * CLASSES - 1) == ERR_CAPACITY and (out == 7).all()
        assert call(cap=length * 2 * CLASSES) == 0
        assert np.array_equal(out[:length * 2 * CLASSES].reshape(length, 2, CLASSES), site_counts(codes, g, 2))
        assert (out[length * 2 * CLASSES:] == 7).all()
        # an empty range writes nothing and needs no room (an empty set cannot be uploaded: "Empty FASTA file")
        out[:] = 7
        assert call(begin=40, end=40, cap=0) == 0 and (out == 7).all()
