"""GPU (-m gpu): dst_site_ld and dst_site_ld_links against site_ld_reference, bitwise: the record shapes around a wave and a
K-step of the tile kernel (8 words = 512 records), the list lengths around a tile (64 positions) with the listed sites at
the edges of the 32-site words and 128-site chunks, every code at listed sites, group selections, caller-supplied alleles,
row ranges, tallies past 65,535, stale padding, a deferring upload, the state the calls must leave alone, every documented
error, and the links at every threshold, slab size and window the compaction distinguishes.  Shapes are the smallest at
which the kernels can go wrong."""
import ctypes as C

import numpy as np
import pytest

import distance_amd as da
from distance_amd import _lib
from helpers import CODES, random_alignment, uniform_codes
from site_ld_reference import finalize, links, pair_index, same_bits, site_major, tallies, tallies_by_products
from site_counts_reference import site_counts
from tools import synth

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE, ERR_CAPACITY = 1, 4, 6
A, T, G, C_, N, R = 136, 24, 72, 40, 240, 192
TILE, KSTEP = 64, 512   # positions of a tile side, records of a K-step (dst_site_ld.hip)
# the edges of the 32-site words and the 128-site chunks, in one chunk and across several
EDGES = [0, 31, 32, 127, 128, 159, 160, 255, 256, 383, 511, 640]


@pytest.fixture(scope="module")
def eng():
    with da.Engine(0) as e:
        yield e


def site_list(S, length, seed=0):
    """S ascending sites of [0, length) that hold the EDGES below length first"""
    edges = [s for s in EDGES if s < length]
    rest = [s for s in np.random.default_rng(seed).permutation(length).tolist() if s not in edges]
    return np.array(sorted((edges + rest)[:S]), np.uint32)


def check(eng, codes, sites, alleles=None, groups=None, which=0, row_begin=0, row_end=None):
    got, used = eng.site_ld(sites, alleles, 0, groups, which, row_begin, row_end)
    if alleles is None:   # the default: the major allele among the participating records
        member = None if groups is None else np.where(np.where(np.asarray(groups) == -1, 0xFFFFFFFF, groups) == which, 0, -1)
        want_alleles = site_major(site_counts(codes, member, 1), 0)[0][np.asarray(sites, np.int64)] if len(sites) else np.zeros(0, np.uint8)
        assert np.array_equal(used, want_alleles), (used, want_alleles)
        alleles = used
    want = tallies(codes, sites, alleles, groups, which, row_begin, row_end)
    assert got.dtype == np.uint32 and got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want), (codes.shape, len(sites), np.argwhere(got != want)[:5].tolist())
    return got


@pytest.mark.parametrize("n", [1, 63, 64, 65, KSTEP - 1, KSTEP, KSTEP + 1])
def test_record_shapes(eng, n):
    length = 700
    codes = random_alignment(n, length, 100 + n, p_ambig=0.05, p_gap=0.1, divergence=0.4)
    eng.upload(0, codes)
    check(eng, codes, site_list(20, length, n))
    check(eng, codes, site_list(20, length, n), groups=np.arange(n) % 3 - 1, which=1)


@pytest.mark.parametrize("S", [0, 1, 2, TILE - 1, TILE, TILE + 1])
def test_list_lengths(eng, S):
    n, length = 130, 1000
    codes = random_alignment(n, length, 7, p_ambig=0.05, p_gap=0.1, divergence=0.4)
    eng.upload(0, codes)
    sites = site_list(S, length, S)
    got = check(eng, codes, sites)
    assert len(got) == S * (S - 1) // 2
    if S == TILE + 1:   # the same list inside ONE chunk and its neighbour: bits 0..64 of chunk 1
        check(eng, codes, np.arange(128, 128 + S, dtype=np.uint32))
        check(eng, codes, np.array(EDGES[:5], np.uint32))
        assert np.array_equal(tallies(codes, sites, np.zeros(S, np.uint8)), tallies_by_products(codes, sites, np.zeros(S, np.uint8)))


def test_every_code_at_listed_sites(eng):
    """column c of record r holds code (r + c) % 17: every listed bit position meets every code"""
    length, n = 2 * 128 + 17, 17 * 4
    codes = CODES[(np.arange(n)[:, None] + np.arange(length)[None, :]) % 17]
    eng.upload(0, codes)
    sites = np.array(sorted(set([s for s in EDGES if s < length] + list(range(120, 140)) + [length - 1])), np.uint32)
    for allele in range(4):
        got = check(eng, codes, sites, np.full(len(sites), allele, np.uint8))
        assert got[:, 0].max() <= 16   # four single-base codes out of 17, four blocks
    check(eng, codes, sites, groups=np.arange(n) // 17, which=2)


def test_group_selections(eng):
    n, length = KSTEP + 90, 400
    codes = random_alignment(n, length, 21, p_ambig=0.1, p_gap=0.1, divergence=0.3)
    eng.upload(0, codes)
    sites = site_list(30, length, 4)
    contiguous = np.minimum(np.arange(n) * 3 // n, 2)
    interleaved = np.arange(n) % 3
    none = np.where(np.arange(n) % 5 == 0, -1, np.arange(n) % 2)
    for g, which in ((contiguous, 0), (contiguous, 2), (interleaved, 1), (none, 0), (none, 1)):
        check(eng, codes, sites, groups=g, which=which)
    # an empty group: zero tallies, no launch; the links are none
    got, _ = eng.site_ld(sites, np.zeros(30, np.uint8), 0, interleaved, 7)
    assert got.shape == (435, 4) and not got.any()
    assert eng.site_ld_links(sites, 0.0, np.zeros(30, np.uint8), 0, interleaved, 7, count_only=True) == 0
    assert len(eng.site_ld_links(sites, 0.0, np.zeros(30, np.uint8), 0, interleaved, 7)[0]) == 0


def test_alleles_of_the_caller(eng):
    n, length = 200, 300
    codes = random_alignment(n, length, 33, p_ambig=0.05, p_gap=0.05, divergence=0.4)
    eng.upload(0, codes)
    sites = site_list(25, length, 5)
    default = check(eng, codes, sites)
    major = site_major(site_counts(codes), 0)[0][sites.astype(np.int64)]
    other = ((major + 1 + np.arange(25) % 3) % 4).astype(np.uint8)   # never the major one
    assert (other != major).all()
    got = check(eng, codes, sites, other)
    assert np.array_equal(got[:, 0], default[:, 0]) and not np.array_equal(got, default)


def test_row_ranges(eng):
    n, length, S = 100, 300, 9
    codes = random_alignment(n, length, 44, p_ambig=0.05, p_gap=0.1, divergence=0.4)
    eng.upload(0, codes)
    sites = site_list(S, length, 6)
    alleles = np.arange(S, dtype=np.uint8) % 4
    whole = check(eng, codes, sites, alleles)
    for cut in range(S + 1):
        first = check(eng, codes, sites, alleles, row_begin=0, row_end=cut)
        second = check(eng, codes, sites, alleles, row_begin=cut, row_end=S)
        assert np.array_equal(np.concatenate([first, second]), whole)
    rows = [check(eng, codes, sites, alleles, row_begin=p, row_end=p + 1) for p in range(S)]
    assert np.array_equal(np.concatenate(rows), whole) and len(rows[-1]) == 0
    # a tile's edge inside the range: 70 positions, rows 60..66
    sites = site_list(70, length, 8)
    alleles = np.zeros(70, np.uint8)
    whole = tallies(codes, sites, alleles)
    at = [e for e, (p, _) in enumerate(pair_index(70)) if 60 <= p < 67]
    got, _ = eng.site_ld(sites, alleles, row_begin=60, row_end=67)
    assert np.array_equal(got, whole[at])


def test_tallies_past_65535(eng):
    n = 70_000
    codes = np.full((n, 130), A, np.uint8)
    codes[n // 2:, 5] = G
    codes[0::2, 129] = T
    codes[:, 64] = N
    eng.upload(0, codes)
    sites, alleles = np.array([5, 64, 129], np.uint32), np.zeros(3, np.uint8)
    got, _ = eng.site_ld(sites, alleles)
    assert got.tolist() == [[0, 0, 0, 0], [n, n // 2, n // 2, n // 4], [0, 0, 0, 0]]
    pi, pj, t, _ = eng.site_ld_links(sites, 0.0, alleles)
    assert pi.tolist() == [0] and pj.tolist() == [2] and t.tolist() == [[n, n // 2, n // 2, n // 4]]


def test_stale_padding_is_not_counted(eng):
    eng.upload(0, np.full((900, 400), A, np.uint8))   # the slot's buffers are kept: whatever the next pack leaves behind
    big = site_list(70, 400, 2)
    eng.site_ld(big, np.full(70, 2, np.uint8))        # ... and the vectors of a longer list over more records
    codes = uniform_codes(65, 129, 3)
    eng.upload(0, codes)
    check(eng, codes, np.array([0, 31, 32, 127, 128], np.uint32))
    check(eng, codes, np.arange(129, dtype=np.uint32)[::2], groups=np.arange(65) % 2, which=1)


def test_after_a_deferring_upload():
    n, length = 2_000, 5_000
    codes = synth.alignment(synth.SEED ^ 77, n, length)
    codes[7, 100:400] = N
    codes[9, ::37] = R
    counts = site_counts(codes)
    variable = np.flatnonzero((counts[:, 0, :4] > 0).sum(axis=1) >= 2).astype(np.uint32)[:40]
    assert len(variable) >= 10
    alleles = site_major(counts, 0)[0][variable.astype(np.int64)]
    with da.Engine(0) as e:
        e.set_prep_threshold(0)
        e.upload(0, codes)
        assert not e.planes_stored(0), "the upload stored every plane: nothing here tests the deferred form"
        check(e, codes, variable, alleles)
        assert e.planes_stored(0)
        check(e, codes, variable, alleles, groups=np.arange(n) % 3, which=2)


def test_leaves_runs_and_the_path_alone(eng):
    codes = random_alignment(300, 900, 4)
    eng.upload(0, codes)
    sites = site_list(40, 900, 1)
    for path in ("dense", "consensus"):
        eng.set_path(path)
        before = {m: eng.run_square(m) for m in ("n", "raw", "tn93")}
        assert eng.last_path() == path
        launch = eng.last_launch()
        check(eng, codes, sites, groups=np.arange(300) % 4, which=3)
        eng.site_ld_links(sites, 0.1, np.zeros(40, np.uint8))
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
        out = []
        for call in (lambda: e.site_ld([1, 2, 3], [0, 0, 0]), lambda: e.site_ld_links([1, 2, 3], 0.5, [0, 0, 0])):
            with pytest.raises(da.DistanceError) as err:
                call()
            out.append((err.value.status, err.value.message))
        return out

    try:
        for result in ThreadRanks(2).run(body):
            for status, message in result:
                assert status == ERR_STATE and "dst_upload_shared runs on the consensus path only" in message
    finally:
        hip.lib.hipFree(d_codes)


def test_errors_in_their_order():
    lib = da.load()
    n, length, S = 9, 300, 5
    codes = uniform_codes(n, length, 2)
    sites = np.array([3, 40, 128, 129, 299], np.uint32)
    alleles = np.array([0, 1, 2, 3, 0], np.uint8)
    g = (np.arange(n) % 2).astype(np.uint32)
    out = np.full(4 * 10 + 8, 7, np.uint32)
    with da.Engine(0) as e:
        h = e._h

        def full(slot=0, s=sites, a=alleles, S_=S, group=g, which=1, rb=0, re=S, tal=out, cap=10):
            return lib.dst_site_ld(h, slot, None if s is None else s.ctypes.data, None if a is None else a.ctypes.data, S_,
                                   None if group is None else group.ctypes.data, which, rb, re,
                                   None if tal is None else tal.ctypes.data, cap)

        def lnk(slot=0, s=sites, a=alleles, S_=S, group=g, which=1, r2=0.5):
            total = C.c_uint64(99)
            rc = lib.dst_site_ld_links(h, slot, None if s is None else s.ctypes.data, None if a is None else a.ctypes.data, S_,
                                       None if group is None else group.ctypes.data, which, r2, 0, None, None, C.byref(total))
            return rc, int(total.value)

        def message():
            return lib.dst_last_error(h).decode()

        # the first tier comes before the set's state: nothing is uploaded yet
        assert full(tal=None) == ERR_ARG and full(s=None) == ERR_ARG and full(a=None) == ERR_ARG
        assert full(slot=2) == ERR_ARG and full(slot=-1) == ERR_ARG
        assert full(group=None, which=1) == ERR_ARG and "which must be 0" in message()
        assert lnk(s=None)[0] == ERR_ARG and lnk(a=None)[0] == ERR_ARG and lnk(slot=2)[0] == ERR_ARG and lnk(group=None)[0] == ERR_ARG
        assert full() == ERR_STATE and "not uploaded" in message() and lnk() == (ERR_STATE, 0)
        e.upload(0, codes)
        assert full(slot=1) == ERR_STATE
        # the list: a site past the end, then the order; the message names the first such position
        bad = sites.copy()
        bad[4] = 300
        assert full(s=bad) == ERR_ARG and "position 4 names site 300" in message() and lnk(s=bad)[0] == ERR_ARG
        bad = sites.copy()
        bad[2], bad[3] = 40, 39
        assert full(s=bad) == ERR_ARG and "position 2 names site 40 after site 40" in message() and "strictly ascending" in message()
        worse = alleles.copy()
        worse[1], worse[3] = 4, 9
        assert full(a=worse) == ERR_ARG and "position 1 has allele 4" in message() and lnk(a=worse)[0] == ERR_ARG
        assert full(s=bad, a=worse) == ERR_ARG and "strictly ascending" in message()       # the list before the alleles
        assert full(rb=3, re=2) == ERR_ARG and full(re=S + 1) == ERR_ARG and "[0, 6)" in message()
        assert full(a=worse, re=S + 1) == ERR_ARG and "allele" in message()                 # the alleles before the range
        assert lnk(r2=float("nan"))[0] == ERR_ARG and "NaN" in message()
        # a bad range before the capacity; the capacity with nothing written
        assert full(re=S + 1, cap=0) == ERR_ARG
        assert full(cap=9) == ERR_CAPACITY and (out == 7).all()
        assert full(rb=1, re=3, cap=4) == ERR_CAPACITY and (out == 7).all()
        assert full(cap=10) == 0
        assert np.array_equal(out[:40].reshape(10, 4), tallies(codes, sites, alleles, g, 1)) and (out[40:] == 7).all()
        out[:] = 7
        assert full(rb=1, re=3, cap=5) == 0
        assert np.array_equal(out[:20].reshape(5, 4), tallies(codes, sites, alleles, g, 1, 1, 3)) and (out[20:] == 7).all()
        # fewer than two sites, an empty row range and the last row alone: DST_OK, nothing written, no room needed
        out[:] = 7
        assert full(S_=1, re=1, cap=0) == 0 and full(S_=0, re=0, cap=0) == 0 and full(rb=2, re=2, cap=0) == 0
        assert full(rb=4, re=5, cap=0) == 0 and (out == 7).all()
        assert lnk(S_=1) == (0, 0) and lnk(S_=0) == (0, 0) and lnk(which=5) == (0, 0)
        # every r2 at or below 0 asks for every pair with a defined r2
        assert lnk(r2=-1.0) == lnk(r2=0.0) == lnk(r2=float("-inf"))
        assert lnk(r2=float("inf")) == (0, 0)


# ---- the links ----------------------------------------------------------------------------------------------------------
def check_links(eng, codes, sites, alleles, min_r2, groups=None, which=0, max_pairs=0):
    pi, pj, t, _ = eng.site_ld_links(sites, min_r2, alleles, 0, groups, which, max_pairs)
    wi, wj, wt = links(codes, sites, alleles, min_r2, groups, which)
    assert np.array_equal(pi, wi) and np.array_equal(pj, wj) and np.array_equal(t, wt), (min_r2, max_pairs, len(pi), len(wi))
    assert eng.site_ld_links(sites, min_r2, alleles, 0, groups, which, max_pairs, count_only=True) == len(wi)
    return len(wi)


@pytest.fixture(scope="module")
def linked():
    """300 records, 70 listed sites (a tile and a bit), sites in correlated blocks so that every threshold keeps some pairs"""
    rng = np.random.default_rng(12)
    n, length = 300, 700
    codes = np.full((n, length), A, np.uint8)
    sites = site_list(70, length, 3)
    base = rng.random((7, n)) < 0.4
    for p, s in enumerate(sites):
        minor = base[p % 7] ^ (rng.random(n) < 0.02 * max(0, p // 7 - 1))   # block p % 7: two exact copies, then noisier ones
        codes[minor, s] = G
        codes[rng.random(n) < 0.05, s] = N
    return codes, sites, np.zeros(70, np.uint8)


@pytest.mark.parametrize("min_r2", [0.0, 0.2, 1.0])
def test_links_at_thresholds(eng, linked, min_r2):
    codes, sites, alleles = linked
    eng.upload(0, codes)
    counts = [check_links(eng, codes, sites, alleles, min_r2, max_pairs=mp) for mp in (0, 1, 200, 69 + 68 + 67)]   # the default, one row, a few rows
    assert len(set(counts)) == 1 and (counts[0] > 0)
    if min_r2 == 0.0:
        assert counts[0] <= 70 * 69 // 2
    check_links(eng, codes, sites, alleles, min_r2, groups=np.arange(300) % 2, which=1, max_pairs=500)


def test_links_at_exactly_a_quarter(eng):
    """8 records: sites 0 and 1 give {8, 4, 4, 3}: r2 = 0.25 exactly, a link at 0.25 and none at the next double"""
    codes = np.full((8, 140), A, np.uint8)
    codes[[0, 1, 2, 3], 0] = G
    codes[[0, 1, 2, 4], 1] = G
    codes[[0, 1, 2, 3], 130] = T        # complete LD with site 0
    codes[[4, 5, 6, 7], 131] = C_       # ... and repulsion
    codes[[0, 2, 4, 6], 139] = G        # independent of site 0
    sites, alleles = np.array([0, 1, 130, 131, 139], np.uint32), np.zeros(5, np.uint8)
    eng.upload(0, codes)
    t, _ = eng.site_ld(sites, alleles)
    assert t[0].tolist() == [8, 4, 4, 3] and finalize(t)["r2"][0] == 0.25
    assert same_bits(da.ld_finalize(t)["r2"], finalize(t)["r2"])
    above = float(np.nextafter(0.25, 1.0))
    at = check_links(eng, codes, sites, alleles, 0.25)
    over = check_links(eng, codes, sites, alleles, above)
    pi, pj, _, _ = eng.site_ld_links(sites, 0.25, alleles)
    assert (0, 1) in list(zip(pi.tolist(), pj.tolist()))
    pi, pj, _, _ = eng.site_ld_links(sites, above, alleles)
    assert (0, 1) not in list(zip(pi.tolist(), pj.tolist())) and over < at
    check_links(eng, codes, sites, alleles, 1.0)


def test_links_past_one_window(eng):
    """3,000 sites of 64 records, every pair with a defined r2: 4,498,500 links, more than one DST_LD_CHUNK window of one
    slab, and two slabs of them at a forced slab size"""
    rng = np.random.default_rng(5)
    n, S = 64, 3000
    codes = np.where(rng.random((n, S)) < 0.5, A, G).astype(np.uint8)
    codes[0], codes[1] = A, G       # every site has both alleles
    sites, alleles = np.arange(S, dtype=np.uint32), np.zeros(S, np.uint8)
    eng.upload(0, codes)
    want = tallies_by_products(codes, sites, alleles)
    assert np.array_equal(want[:S - 1], tallies(codes, sites, alleles, row_begin=0, row_end=1))
    i, j = np.triu_indices(S, 1)
    pairs = S * (S - 1) // 2
    assert pairs > da.LD_CHUNK
    for max_pairs, calls in ((0, [da.LD_CHUNK, pairs - da.LD_CHUNK]), (3_000_000, None)):
        pi, pj, t, _ = eng.site_ld_links(sites, 0.0, alleles, max_pairs=max_pairs)
        assert len(pi) == pairs and np.array_equal(pi, i.astype(np.uint32)) and np.array_equal(pj, j.astype(np.uint32))
        assert np.array_equal(t, want)
        assert eng.last_ld_first == np.cumsum([0] + eng.last_ld_calls[:-1]).tolist()
        if calls:
            assert eng.last_ld_calls == calls
        else:
            assert len(eng.last_ld_calls) == 2 and max(eng.last_ld_calls) <= 3_000_000
    assert eng.site_ld_links(sites, 0.0, alleles, count_only=True) == pairs


def test_a_sink_that_stops_the_run(eng, linked):
    codes, sites, alleles = linked
    eng.upload(0, codes)
    lib = da.load()
    seen = []

    def stop(_user, first, count, _i, _j, _t):
        seen.append((int(first), int(count)))
        return 1 if len(seen) == 2 else 0

    cb = _lib.LD_SINK(stop)
    total = C.c_uint64()
    rc = lib.dst_site_ld_links(eng._h, 0, sites.ctypes.data, alleles.ctypes.data, 70, None, 0, 0.0, 300, cb, None, C.byref(total))
    assert rc == ERR_STATE and "stopped by sink" in lib.dst_last_error(eng._h).decode()
    assert len(seen) == 2 and seen[1][0] == seen[0][1] and int(total.value) == seen[0][1]
    check_links(eng, codes, sites, alleles, 0.2)   # the context serves the next call
