"""GPU (-m gpu): dst_site_ld_band, dst_site_ld_links_band and dst_site_ld_decay, bitwise against Engine.site_ld / site_ld_links /
ld_finalize of the same context, filtered and reduced by site_ld_band_reference.  No tolerance anywhere.  The shapes are the
smallest at which the band kernels can go wrong: list lengths around one and two tiles (64 positions), record counts around
a wave and a K-step (512 records), bands that are empty, one site wide, cut inside a tile, end exactly on a tile's edge and
hold the whole triangle, rows with an empty band (a desert behind a cluster), slabs of one row and slabs that cut a tile
row, bins that a tile gathers on chip (its span at most DST_LD_DECAY_LOCAL_BINS) and bins it adds to memory directly."""
import ctypes as C

import numpy as np
import pytest

import distance_amd as da
from distance_amd import _lib
from helpers import CODES, random_alignment, uniform_codes
from site_ld_band_reference import band_mask, band_pairs, band_rows, decay, links_in_band, same_curve
from site_ld_reference import tallies, tallies_by_products
from tools import synth

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE, ERR_CAPACITY = 1, 4, 6
A, T, G, C_, N, R = 136, 24, 72, 40, 240, 192
TILE, KSTEP = 64, 512
LENGTH = 2600                      # sites of the alignments below
LENGTHS = [2, 63, 64, 65, 129, 200]
RECORDS = [1, 64, 65, 511, 512, 513]


@pytest.fixture(scope="module")
def eng():
    with da.Engine(0) as e:
        yield e


def site_lists(S):
    """regular spacing; clusters (random); a cluster of up to 70 adjacent sites, a desert, then the rest"""
    rng = np.random.default_rng(S)
    regular = np.arange(S, dtype=np.uint32) * 3 + 1
    clustered = np.sort(rng.choice(LENGTH // 2, S, replace=False)).astype(np.uint32)
    head = min(S, 70)
    desert = np.concatenate([np.arange(head), 2000 + 2 * np.arange(S - head)]).astype(np.uint32)
    return {"regular": regular, "clustered": clustered, "desert": desert}


def gaps_of(sites):
    """0, 1, a band that cuts inside a tile, one whose first row ends exactly on the tile's edge, the span and beyond"""
    s = sites.astype(np.int64)
    inside = int(s[min(10, len(s) - 1)] - s[0])
    edge = int(s[min(TILE - 1, len(s) - 1)] - s[0])
    return [0, 1, inside, edge, int(s[-1] - s[0]), 1 << 40]


def check_band(eng, sites, max_gap, full, groups=None, which=0, row_begin=0, row_end=None):
    alleles = np.zeros(len(sites), np.uint8)
    got, _ = eng.site_ld_band(sites, max_gap, alleles, 0, groups, which, row_begin, row_end)
    at = [e for e, (p, _) in enumerate(band_pairs(sites, 1 << 62)) if row_begin <= p < (len(sites) if row_end is None else row_end)]
    want = full[at][band_mask(sites, max_gap, row_begin, row_end)]
    assert got.dtype == np.uint32 and got.shape == want.shape, (len(sites), max_gap, got.shape, want.shape)
    assert np.array_equal(got, want), (len(sites), max_gap, np.argwhere(got != want)[:5].tolist())


def check_links(eng, sites, max_gap, min_r2, unbanded, groups=None, which=0, max_pairs=0):
    alleles = np.zeros(len(sites), np.uint8)
    pi, pj, t, _ = eng.site_ld_links(sites, min_r2, alleles, 0, groups, which, max_pairs, max_gap=max_gap)
    wi, wj, wt = links_in_band(sites, max_gap, *unbanded)
    assert np.array_equal(pi, wi) and np.array_equal(pj, wj) and np.array_equal(t, wt), (len(sites), max_gap, min_r2, max_pairs, len(pi), len(wi))
    assert eng.site_ld_links(sites, min_r2, alleles, 0, groups, which, max_pairs, count_only=True, max_gap=max_gap) == len(wi)
    return len(wi)


def check_decay(eng, sites, width, bins, min_r2, full, groups=None, which=0, max_pairs=0):
    alleles = np.zeros(len(sites), np.uint8)
    got = eng.site_ld_decay(sites, width, bins, min_r2, alleles, 0, groups, which, max_pairs)
    want = decay(sites, full, width, bins, min_r2, r2=da.ld_finalize(full)["r2"])
    assert same_curve(got, want), (len(sites), width, bins, min_r2, max_pairs, {k: np.flatnonzero(got[k] != want[k])[:4].tolist() for k in ("pairs", "defined", "links", "r2_sum")})
    return got


def linked_codes(n, seed):
    """n records over LENGTH sites: columns in correlated blocks (every threshold keeps some pairs), some N, R and gaps"""
    rng = np.random.default_rng(seed)
    base = rng.random((9, n)) < 0.4
    codes = np.full((n, LENGTH), A, np.uint8)
    for s in range(LENGTH):
        minor = base[s % 9] ^ (rng.random(n) < 0.03 * (s % 4))
        codes[minor, s] = G
    codes[rng.random((n, LENGTH)) < 0.04] = N
    codes[rng.random((n, LENGTH)) < 0.01] = R
    return codes


# ---- the full band form and the banded links ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", RECORDS)
def test_band_and_links_at_record_shapes(eng, n):
    """every list length x list shape x band at one record count: the full form, its row ranges, and the links at 0.2"""
    codes = linked_codes(n, 300 + n)
    eng.upload(0, codes)
    for S in LENGTHS:
        for name, sites in site_lists(S).items():
            alleles = np.zeros(S, np.uint8)
            full, _ = eng.site_ld(sites, alleles)
            unbanded = eng.site_ld_links(sites, 0.2, alleles)[:3]
            for max_gap in gaps_of(sites):
                check_band(eng, sites, max_gap, full)
                check_links(eng, sites, max_gap, 0.2, unbanded)
            # the band that holds the triangle is the unbanded call's output, array for array
            pi, pj, t, _ = eng.site_ld_links(sites, 0.2, alleles, max_gap=int(sites[-1] - sites[0]))
            assert np.array_equal(pi, unbanded[0]) and np.array_equal(pj, unbanded[1]) and np.array_equal(t, unbanded[2]), (S, name)
            got, _ = eng.site_ld_band(sites, int(sites[-1] - sites[0]), alleles)
            assert np.array_equal(got, full)


def test_every_code_at_listed_sites(eng):
    """column c of record r holds code (r + c) % 17: every listed bit position meets every code"""
    length, n = 2 * 128 + 17, 17 * 4
    codes = CODES[(np.arange(n)[:, None] + np.arange(length)[None, :]) % 17]
    eng.upload(0, codes)
    sites = np.arange(0, length, 2, dtype=np.uint32)   # 137 positions
    for allele in range(4):
        alleles = np.full(len(sites), allele, np.uint8)
        full, _ = eng.site_ld(sites, alleles)
        want = full[band_mask(sites, 40)]
        got, _ = eng.site_ld_band(sites, 40, alleles)
        assert np.array_equal(got, want) and want[:, 0].max() <= 16
        assert np.array_equal(want, tallies(codes, sites, alleles)[band_mask(sites, 40)])   # (and the plain loops agree)


def test_groups_row_ranges_and_thresholds(eng):
    n, S = 300, 129
    codes = linked_codes(n, 5)
    eng.upload(0, codes)
    groups = np.where(np.arange(n) % 7 == 0, -1, np.arange(n) % 3)
    for name, sites in site_lists(S).items():
        alleles = np.zeros(S, np.uint8)
        inside, edge = gaps_of(sites)[2:4]
        for g, which in ((None, 0), (groups, 1), (groups, 2)):
            full, _ = eng.site_ld(sites, alleles, 0, g, which)
            for max_gap in (inside, edge):
                check_band(eng, sites, max_gap, full, g, which)
                for rb, re in ((0, 1), (60, 67), (63, 64), (64, S), (S - 1, S), (5, 5)):
                    check_band(eng, sites, max_gap, full, g, which, rb, re)
            for min_r2 in (0.0, 0.2, 1.0):
                unbanded = eng.site_ld_links(sites, min_r2, alleles, 0, g, which)[:3]
                # the default slab, one row per slab, a slab that cuts a tile row (row 0's band and a bit)
                row0 = int(band_rows(sites, edge)[0]) - 1
                counts = {check_links(eng, sites, edge, min_r2, unbanded, g, which, mp) for mp in (0, 1, row0 + row0 // 2, 1000)}
                assert len(counts) == 1
                if min_r2 < 1.0 and name != "desert":
                    assert counts.pop() > 0
        # an empty group: zero tallies, no links, no launch
        got, _ = eng.site_ld_band(sites, edge, alleles, 0, groups, 9)
        assert len(got) == int(band_mask(sites, edge).sum()) and not got.any()
        assert eng.site_ld_links(sites, 0.0, alleles, 0, groups, 9, count_only=True, max_gap=edge) == 0


def test_links_past_one_window(eng):
    """3,000 sites of 64 records, every pair with a defined r2, a band of 2,400 sites: 4,318,800 links, more than one
    DST_LD_CHUNK window of one slab, and two slabs of them at a forced slab size"""
    rng = np.random.default_rng(5)
    n, S, max_gap = 64, 3000, 2400
    codes = np.where(rng.random((n, S)) < 0.5, A, G).astype(np.uint8)
    codes[0], codes[1] = A, G       # every site has both alleles
    sites, alleles = np.arange(S, dtype=np.uint32), np.zeros(S, np.uint8)
    eng.upload(0, codes)
    i, j = np.triu_indices(S, 1)
    keep = (j - i) <= max_gap
    want = tallies_by_products(codes, sites, alleles)[keep]
    i, j = i[keep].astype(np.uint32), j[keep].astype(np.uint32)
    pairs = int(keep.sum())
    assert pairs == da.ld_band(sites, max_gap)[1] and pairs > da.LD_CHUNK
    for max_pairs, calls in ((0, [da.LD_CHUNK, pairs - da.LD_CHUNK]), (3_000_000, None)):
        pi, pj, t, _ = eng.site_ld_links(sites, 0.0, alleles, max_pairs=max_pairs, max_gap=max_gap)
        assert len(pi) == pairs and np.array_equal(pi, i) and np.array_equal(pj, j) and np.array_equal(t, want)
        assert eng.last_ld_first == np.cumsum([0] + eng.last_ld_calls[:-1]).tolist()
        if calls:
            assert eng.last_ld_calls == calls
        else:
            assert len(eng.last_ld_calls) == 2 and max(eng.last_ld_calls) <= 3_000_000
    assert eng.site_ld_links(sites, 0.0, alleles, count_only=True, max_gap=max_gap) == pairs


def test_a_sink_that_stops_the_run(eng):
    codes = linked_codes(300, 8)
    eng.upload(0, codes)
    sites = site_lists(129)["regular"]
    alleles = np.zeros(129, np.uint8)
    lib = da.load()
    seen = []

    def stop(_user, first, count, _i, _j, _t):
        seen.append((int(first), int(count)))
        return 1 if len(seen) == 2 else 0

    cb = _lib.LD_SINK(stop)
    total = C.c_uint64()
    rc = lib.dst_site_ld_links_band(eng._h, 0, sites.ctypes.data, alleles.ctypes.data, 129, None, 0, 0.0, 60, 300, cb, None, C.byref(total))
    assert rc == ERR_STATE and "stopped by sink" in lib.dst_last_error(eng._h).decode()
    assert len(seen) == 2 and seen[1][0] == seen[0][1] and int(total.value) == seen[0][1]
    check_links(eng, sites, 60, 0.2, eng.site_ld_links(sites, 0.2, alleles)[:3])   # the context serves the next call


# ---- the decay curve ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", RECORDS)
def test_decay_at_record_shapes(eng, n):
    codes = linked_codes(n, 600 + n)
    eng.upload(0, codes)
    for S in LENGTHS:
        for name, sites in site_lists(S).items():
            alleles = np.zeros(S, np.uint8)
            full, _ = eng.site_ld(sites, alleles)
            span = int(sites[-1] - sites[0])
            for width, bins in ((1, 4096), (1, 1), (7, 13), (span + 1, 1)):
                got = check_decay(eng, sites, width, bins, 0.2, full)
            # one bin over everything: site_ld_links' count-only totals at 0 and at R2
            assert int(got["pairs"][0]) == S * (S - 1) // 2
            assert int(got["links"][0]) == eng.site_ld_links(sites, 0.2, alleles, count_only=True)
            all_defined = eng.site_ld_links(sites, 0.0, alleles, count_only=True)
            got = check_decay(eng, sites, span + 1, 1, 0.0, full)
            assert int(got["defined"][0]) == int(got["links"][0]) == all_defined


def test_decay_on_chip_and_in_memory(eng):
    """regular spacing 3 at width 7: a tile spans 2 x 64 x 3 / 7 = 55 bins at most, gathered on chip.  Spacing 10 at width 1:
    a diagonal tile spans 630 bins and the others more, past DST_LD_DECAY_LOCAL_BINS = 512: added to memory directly.  Both in
    groups, and whatever max_pairs cuts the launches into."""
    assert da.LD_DECAY_LOCAL_BINS == 512
    n, S = 200, 200
    codes = linked_codes(n, 11)
    eng.upload(0, codes)
    groups = np.arange(n) % 2
    narrow, spread = np.arange(S, dtype=np.uint32) * 3, np.arange(S, dtype=np.uint32) * 10
    assert 2 * TILE * 3 // 7 < da.LD_DECAY_LOCAL_BINS < (TILE - 1) * 10
    for sites, width, bins in ((narrow, 7, 60), (narrow, 7, 4096), (spread, 1, 4096), (spread, 1, 700), (spread, 2, 900)):
        for g, which in ((None, 0), (groups, 1)):
            full, _ = eng.site_ld(sites, np.zeros(S, np.uint8), 0, g, which)
            curves = [check_decay(eng, sites, width, bins, 0.2, full, g, which, mp) for mp in (0, 1, 5000)]
            assert int(curves[0]["defined"].sum()) > 0 and int(curves[0]["links"].sum()) > 0
            assert int(curves[0]["pairs"].sum()) == da.ld_band(sites, width * bins - 1)[1]


def test_decay_of_duplicated_columns(eng):
    """every listed site holds the same column, but for one monomorphic site: every defined pair has r2 = 1, so r2_sum ==
    defined exactly, in every bin"""
    rng = np.random.default_rng(3)
    n, S = 150, 130
    column = np.where(rng.random(n) < 0.3, G, A).astype(np.uint8)
    codes = np.repeat(column[:, None], 400, axis=1)
    codes[:, 100] = A
    eng.upload(0, codes)
    sites = np.arange(40, 40 + S, dtype=np.uint32)
    full, _ = eng.site_ld(sites, np.zeros(S, np.uint8))
    for width, bins in ((1, 200), (16, 4), (1000, 1)):
        got = check_decay(eng, sites, width, bins, 1.0, full)
        assert np.array_equal(got["r2_sum"], got["defined"].astype(np.float64)) and np.array_equal(got["links"], got["defined"])
        assert int(got["defined"].sum()) > 0 and int((got["pairs"] - got["defined"]).sum()) > 0


def test_decay_tallies_past_65535(eng):
    n = 70_000
    codes = np.full((n, 130), A, np.uint8)
    codes[n // 2:, 5] = G
    codes[0::2, 129] = T
    codes[: n // 4, 129] = T
    codes[:, 64] = N
    eng.upload(0, codes)
    sites, alleles = np.array([5, 64, 129], np.uint32), np.zeros(3, np.uint8)
    full, _ = eng.site_ld(sites, alleles)
    assert int(full[1, 0]) == n and int(full[1, 3]) > 65535 // 4
    got = check_decay(eng, sites, 100, 2, 0.0, full)
    assert got["pairs"].tolist() == [2, 1] and got["defined"].tolist() == [0, 1]
    band, _ = eng.site_ld_band(sites, 124, alleles)
    assert np.array_equal(band, full)


def test_after_a_deferring_upload():
    n, length = 2_000, 5_000
    codes = synth.alignment(synth.SEED ^ 77, n, length)
    codes[7, 100:400] = N
    from site_counts_reference import site_counts
    counts = site_counts(codes)
    variable = np.flatnonzero((counts[:, 0, :4] > 0).sum(axis=1) >= 2).astype(np.uint32)[:40]
    assert len(variable) >= 10
    for call in range(3):
        with da.Engine(0) as e:
            e.set_prep_threshold(0)
            e.upload(0, codes)
            assert not e.planes_stored(0), "the upload stored every plane: nothing here tests the deferred form"
            alleles = np.zeros(len(variable), np.uint8)
            gap = int(variable[5] - variable[0])
            if call == 0:
                got, _ = e.site_ld_band(variable, gap, alleles)
            elif call == 1:
                got = e.site_ld_links(variable, 0.0, alleles, max_gap=gap)
            else:
                got = e.site_ld_decay(variable, 50, 40, 0.1, alleles)
            assert e.planes_stored(0)
            full, _ = e.site_ld(variable, alleles)
            if call == 0:
                assert np.array_equal(got, full[band_mask(variable, gap)])
            elif call == 1:
                want = links_in_band(variable, gap, *e.site_ld_links(variable, 0.0, alleles)[:3])
                assert all(np.array_equal(x, y) for x, y in zip(got[:3], want))
            else:
                assert same_curve(got, decay(variable, full, 50, 40, 0.1, r2=da.ld_finalize(full)["r2"]))


def test_leaves_runs_and_the_path_alone(eng):
    codes = random_alignment(300, 900, 4)
    eng.upload(0, codes)
    sites = np.sort(np.random.default_rng(1).choice(900, 70, replace=False)).astype(np.uint32)
    alleles = np.zeros(70, np.uint8)
    for path in ("dense", "consensus"):
        eng.set_path(path)
        before = {m: eng.run_square(m) for m in ("n", "raw", "tn93")}
        assert eng.last_path() == path
        launch = eng.last_launch()
        eng.site_ld_band(sites, 100, alleles)
        eng.site_ld_links(sites, 0.1, alleles, max_gap=100)
        eng.site_ld_decay(sites, 10, 20, 0.1, alleles, groups=np.arange(300) % 4, which=3)
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
        out = []
        for call in (lambda: e.site_ld_band([1, 2, 3], 5, [0, 0, 0]), lambda: e.site_ld_links([1, 2, 3], 0.5, [0, 0, 0], max_gap=5),
                     lambda: e.site_ld_decay([1, 2, 3], 1, 4, 0.5, [0, 0, 0])):
            with pytest.raises(da.DistanceError) as err:
                call()
            out.append((err.value.status, err.value.message))
        return out

    try:
        for result in ThreadRanks(2).run(body):
            assert len(result) == 3
            for status, message in result:
                assert status == ERR_STATE and "dst_upload_shared runs on the consensus path only" in message
    finally:
        hip.lib.hipFree(d_codes)


def test_a_band_past_2_33_pairs_is_refused(eng):
    """131,073 sites in one bin are 2^33 + 65,536 pairs: refused on the host, before the room is looked at; 131,072 sites
    (2^33 - 65,536 pairs) pass the check (no record takes part: no launch, the pairs filled)"""
    S = 131_073
    eng.upload(0, np.full((2, S), A, np.uint8))
    sites, alleles = np.arange(S, dtype=np.uint32), np.zeros(S, np.uint8)
    bins = (_lib.LdBin * 1)()
    lib = da.load()

    def dec(S_, width, n_bins, cap, which):
        labels = np.zeros(2, np.uint32)
        return lib.dst_site_ld_decay(eng._h, 0, sites.ctypes.data, alleles.ctypes.data, S_, labels.ctypes.data, which, 0.0, width, n_bins, 0,
                                     C.addressof(bins), cap)

    assert S * (S - 1) // 2 > 1 << 33 > (S - 1) * (S - 2) // 2
    assert dec(S, 1 << 20, 1, 0, 5) == ERR_ARG and "2^33" in lib.dst_last_error(eng._h).decode()
    assert dec(S, 65_536, 2, 2, 5) == ERR_ARG   # (in two bins as well: the band is what counts)
    assert dec(S - 1, 1 << 20, 1, 0, 5) == ERR_CAPACITY
    assert dec(S - 1, 1 << 20, 1, 1, 5) == 0 and bins[0].pairs == (S - 1) * (S - 2) // 2 and bins[0].defined == 0
    assert dec(S, 1000, 1, 1, 5) == 0 and bins[0].pairs == da.ld_band(sites, 999)[1]   # a narrow band of the long list is fine


def test_errors_in_their_order():
    lib = da.load()
    n, length, S = 9, 300, 5
    codes = uniform_codes(n, length, 2)
    sites = np.array([3, 40, 128, 129, 299], np.uint32)
    alleles = np.array([0, 1, 2, 3, 0], np.uint8)
    g = (np.arange(n) % 2).astype(np.uint32)
    out = np.full(4 * 10 + 8, 7, np.uint32)
    curve = (_lib.LdBin * 8)()
    with da.Engine(0) as e:
        h = e._h

        def ptr(x):
            return None if x is None else x.ctypes.data

        def full(slot=0, s=sites, a=alleles, S_=S, group=g, which=1, gap=100, rb=0, re=S, tal=out, cap=10):
            return lib.dst_site_ld_band(h, slot, ptr(s), ptr(a), S_, ptr(group), which, gap, rb, re, ptr(tal), cap)

        def lnk(slot=0, s=sites, a=alleles, S_=S, group=g, which=1, r2=0.5, gap=100):
            total = C.c_uint64(99)
            rc = lib.dst_site_ld_links_band(h, slot, ptr(s), ptr(a), S_, ptr(group), which, r2, gap, 0, None, None, C.byref(total))
            return rc, int(total.value)

        def dec(slot=0, s=sites, a=alleles, S_=S, group=g, which=1, r2=0.5, width=10, bins=8, to=curve, cap=8):
            return lib.dst_site_ld_decay(h, slot, ptr(s), ptr(a), S_, ptr(group), which, r2, width, bins, 0,
                                         None if to is None else C.addressof(to), cap)

        def message():
            return lib.dst_last_error(h).decode()

        # the first tier comes before the set's state: nothing is uploaded yet
        assert full(tal=None) == ERR_ARG and dec(to=None) == ERR_ARG and "null bins pointer" in message()
        for call in (full, dec, lambda **k: lnk(**k)[0]):
            assert call(s=None) == ERR_ARG and call(a=None) == ERR_ARG and call(slot=2) == ERR_ARG
            assert call(group=None, which=1) == ERR_ARG and "which must be 0" in message()
            assert call() == ERR_STATE and "not uploaded" in message()
        e.upload(0, codes)
        bad = sites.copy()
        bad[2], bad[3] = 40, 39
        worse = alleles.copy()
        worse[1] = 4
        for call, name in ((full, "site ld band"), (dec, "site ld decay"), (lambda **k: lnk(**k)[0], "site ld links band")):
            assert call(slot=1) == ERR_STATE
            assert call(s=bad) == ERR_ARG and message().startswith(name + ": position 2 names site 40 after site 40")
            assert call(a=worse) == ERR_ARG and message().startswith(name + ": position 1 has allele 4")
            assert call(s=bad, a=worse) == ERR_ARG and "strictly ascending" in message()
        assert full(rb=3, re=2) == ERR_ARG and full(re=S + 1) == ERR_ARG and "[0, 6)" in message()
        assert full(re=S + 1, cap=0) == ERR_ARG
        # the decay call's own: NaN, the width, the bins, then the room
        nan = float("nan")
        assert lnk(r2=nan)[0] == ERR_ARG and "NaN" in message()
        assert dec(a=worse, r2=nan) == ERR_ARG and "allele" in message()
        assert dec(r2=nan, width=0) == ERR_ARG and "NaN" in message()
        assert dec(width=0, bins=0) == ERR_ARG and "bin_width" in message()
        assert dec(bins=0, cap=0) == ERR_ARG and "n_bins" in message() and dec(bins=4097) == ERR_ARG and "4097" in message()
        assert dec(cap=7) == ERR_CAPACITY and dec(bins=4096, cap=8) == ERR_CAPACITY
        # the capacity of the full form counts band pairs, and nothing is written
        band = int(band_mask(sites, 100).sum())
        assert band == 4 and full(cap=3) == ERR_CAPACITY and (out == 7).all()
        assert full(cap=4) == 0
        assert np.array_equal(out[:16].reshape(4, 4), tallies(codes, sites, alleles, g, 1)[band_mask(sites, 100)]) and (out[16:] == 7).all()
        # nothing to launch: DST_OK, the pairs filled
        out[:] = 7
        assert full(gap=0, cap=0) == 0 and full(S_=1, re=1, cap=0) == 0 and full(S_=0, re=0, cap=0) == 0 and (out == 7).all()
        assert lnk(gap=0) == (0, 0) and lnk(S_=1) == (0, 0) and lnk(which=5) == (0, 0)
        assert dec(which=5) == 0
        assert [b.pairs for b in curve] == decay(sites, np.zeros((10, 4), np.uint32), 10, 8, 0.5)["pairs"].tolist()
        assert all(b.defined == 0 and b.links == 0 and b.r2_sum == 0.0 for b in curve)
        assert dec(S_=1) == 0 and all(b.pairs == 0 for b in curve)
        assert dec(width=1 << 40, bins=1, cap=1) == 0 and curve[0].pairs == 10
