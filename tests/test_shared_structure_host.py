"""CPU: the designed sets of shared_structure_cases.py hold every list length, range skip, rank cut and block fit that
test_gpu_shared_structure.py relies on — counted from the code matrix alone — and the design is tied to the oracle.

The constants restated here are the engine's: shares of ceil(n / world) rounded up to 256 (shared_layout, checked against
dst_shared_range), a first block capacity of 96 entries per record of a share plus 16,384 and 1.25 x the largest block
plus 4,096 afterwards (dst_shared.cpp), ranges of 1,024 sites and 64 entries a round (range_marks_kernel), the
512-record sample, kHotPermille 50, the 8 % gate and the hot weight of 0.5 beyond which a shared upload falls back."""
import numpy as np
import pytest

import distance_amd as da
import list_structure_cases as ls
import oracle
import shared_structure_cases as sc

FAMILIES = ("n_high", "raw", "k80", "tn93")


def view(codes):
    ref, dev, hot = ls.sampled_reference(codes)
    return ref, dev, hot, ls.census(codes, ref)


@pytest.fixture(scope="module")
def cut():
    codes, names = sc.cut_set()
    return (codes, names) + view(codes)


@pytest.fixture(scope="module")
def cooled():
    codes, names = sc.cooled_census()
    return (codes, names) + view(codes)


@pytest.fixture(scope="module")
def wide():
    codes, names = sc.wide_cut_set()
    return (codes, names) + view(codes)


def rides_the_shared_path(codes, dev, hot, c, worlds):
    """below the 8 % gate, hot weight at most 0.5, and every rank's share within the first upload's block"""
    n, L = codes.shape
    samples = min(n, 512)
    assert int(dev.sum()) <= int(0.08 * L * samples)
    assert sc.hot_weight(dev, hot, samples) <= 0.5
    for world in worlds:
        assert max(sc.share_totals(c["length"], n, world)) <= sc.first_capacity(n, world), world


def test_rank_cuts_are_the_engines():
    assert [e - b for b, e in sc.shares(1100, 2)] == [768, 332]
    assert [e - b for b, e in sc.shares(1100, 3)] == [512, 512, 76]
    assert [e - b for b, e in sc.shares(1100, 4)] == [512, 512, 76, 0]
    assert [e - b for b, e in sc.shares(1100, 5)] == [256, 256, 256, 256, 76]
    assert [e - b for b, e in sc.shares(2, 2)] == [2, 0]
    assert [e - b for b, e in sc.shares(257, 2)] == [256, 1]
    assert [e - b for b, e in sc.shares(300, 3)] == [256, 44, 0]
    assert [e - b for b, e in sc.shares(512, 2)] == [256, 256]
    assert sc.shares(4396, 2) == [(0, 2304), (2304, 4396)] and sc.shares(4396, 3) == [(0, 1536), (1536, 3072), (3072, 4396)]
    for n in (2, 257, 300, 512, 600, 722, 1100, 4396):
        for world in (1, 2, 3, 4, 5):
            assert sc.shares(n, world) == [da.shared_range(n, k, world) for k in range(world)], (n, world)
    assert sc.first_capacity(512, 2) == 256 * 96 + 16384 == 40960 == sc.FIT_CAPACITY


def test_cut_set_shape_and_gates(cut):
    codes, names, ref, dev, hot, c = cut
    assert codes.shape == (1100, 4200)
    assert -(-4200 // 1024) == 5 and 4200 - 4 * 1024 == 104 and -(-4200 // 128) == 33
    assert np.array_equal(ref, names["root"] >> 4)               # the root is the plurality at every site
    assert int(hot.sum()) == 0 and int(dev.max()) <= 25           # no hot site: at most 25 of the 512 sampled deviate
    rides_the_shared_path(codes, dev, hot, c, (2, 3, 4, 5))
    assert ls.run_record_count(c["run_chunks"]) == 0


def test_cut_set_features_sit_either_side_of_every_cut(cut):
    codes, names, ref, dev, hot, c = cut
    feat = names["features"]
    for world in (2, 3, 4, 5):
        for b, e in sc.shares(1100, world):
            if 0 < b < 1100:
                assert b - 1 in feat and b in feat, (world, b)
    assert 1099 in feat and set(sc.CUT_RECORDS) <= set(feat)
    cuts = {256, 512, 768, 1024}
    # one record per feature inside a share, at least seven records from every cut
    assert sorted(names["mid"]) == sorted(sc.FEATURES) and len(set(names["mid"].values())) == 17
    for f, r in names["mid"].items():
        assert feat[r] == f and min(abs(r - b) for b in cuts) >= 8 and min(abs(r - b + 1) for b in cuts) >= 7
    assert len(feat) == 26
    plain = [r for r in range(1100) if r not in feat]
    assert np.all(c["length"][plain] == 3)


def test_cut_set_lists_hold_the_named_entries(cut):
    codes, names, ref, dev, hot, c = cut
    length, per_range, per_chunk = c["length"], c["per_range"], c["per_chunk"]
    want_at_cuts = {255: 64, 256: 65, 511: 0, 512: 63, 767: 128, 768: 129, 1099: 193}
    assert {r: int(length[r]) for r in want_at_cuts} == want_at_cuts
    seen = set()
    for r, (kind, k) in names["features"].items():
        if kind == "length":
            assert int(length[r]) == k, r
            seen.add(k)
        elif kind == "ranges_0_and_4":
            assert [int(x) for x in per_range[r]] == [5, 0, 0, 0, 3], r
        elif kind == "range_4_only":
            assert [int(x) for x in per_range[r]] == [0, 0, 0, 0, 6] and c["diff"][r, 4199], r
            assert int(per_chunk[r, 32]) == 6                      # all of it in the 104-site tail
        elif kind == "range_0_only":
            assert [int(x) for x in per_range[r]] == [9, 0, 0, 0, 0], r
        elif kind == "chunk":
            assert int(per_chunk[r, sc.FEATURE_CHUNK]) == k == int(length[r]), r
        elif kind == "chunk_of_n":
            assert np.all(codes[r, 20 * 128:21 * 128] >> 4 == 15) and int(c["run_chunks"][r]) == 1
            assert int(per_chunk[r, 20]) == 120 == int(length[r])   # the chunk's eight N-class sites make no entry
        elif kind == "piece":
            assert [int(x) for x in per_range[r]] == [0, 0, 73, 0, 0], r
    # the 64-lane rounds of range_marks_kernel: none, one, one short of / at / one past one and two rounds, three and one
    assert seen == {0, 1, 63, 64, 65, 127, 128, 129, 193}
    kinds = {k for k in names["features"].values()}
    assert {("chunk", 7), ("chunk", 8), ("chunk", 9)} <= kinds and ls.SLOT_ENTRIES == 7
    # the long lists lie in several ranges each: their marks are all different
    for r, (kind, k) in names["features"].items():
        if kind == "length" and k >= 63:
            assert int((per_range[r] > 0).sum()) == 5, r


def test_fit_sets_fill_the_first_block_to_the_entry():
    fits, over, names = sc.fit_sets()
    assert fits.shape == over.shape == (512, 4200)
    a, b = view(fits), view(over)
    assert sc.share_totals(a[3]["length"], 512, 2) == [40960, 768]
    assert sc.share_totals(b[3]["length"], 512, 2) == [40961, 768]
    assert np.all(a[3]["length"][:256] == 160) and np.all(a[3]["length"][256:] == 3)
    where = np.argwhere(fits != over)
    assert where.tolist() == [[255, names["extra_site"]]] and int(b[3]["length"][255]) == 161
    for ref, dev, hot, c in (a, b):
        assert np.array_equal(ref, names["root"] >> 4)
        assert int(hot.sum()) == 0 and int(dev.max()) <= 25       # no site with 26 or more of the 512 records
        assert int(dev.sum()) <= int(0.08 * 4200 * 512) == 172032
        assert sc.hot_weight(dev, hot, 512) == 0.0
    # 40,960 fits the first block (total > capacity is what falls back), 40,961 does not; what the next upload is given
    assert 40960 <= sc.first_capacity(512, 2) < 40961
    assert sc.next_capacity(40961) >= 40961 and sc.next_capacity(40960) >= 40960
    # a block sized from cut_set's first 512 records is too small for either
    small = view(sc.cut_set()[0][:512])
    biggest = max(sc.share_totals(small[3]["length"], 512, 2))
    assert 0 < biggest and sc.next_capacity(biggest) < 40960
    assert int(small[2].sum()) == 0 and biggest <= sc.first_capacity(512, 2)


def test_the_cooled_census_rides_and_the_census_falls_back(cooled):
    codes, names, ref, dev, hot, c = cooled
    assert codes.shape == (4396, 4200) and np.array_equal(ref, names["root"] >> 4)
    assert int(hot.sum()) == 0 and sc.hot_weight(dev, hot, 512) == 0.0
    rides_the_shared_path(codes, dev, hot, c, (2, 3))
    # the census itself: below the gate, but four sites with 238 or 239 of the 512 sampled records and two with 34 or 35
    census, cnames = ls.census_alignment()
    cref, cdev, chot, _ = view(census)
    assert int(cdev.sum()) <= int(0.08 * 4200 * 512)
    assert sorted(int(x) for x in cdev[chot]) == [34, 35, 238, 239, 239, 239]
    assert sc.hot_weight(cdev, chot, 512) == (238 ** 2 + 3 * 239 ** 2 + 34 ** 2 + 35 ** 2) / 512 ** 2 > 0.5
    # cooling touched the six columns only, and not the record of N
    changed = np.nonzero((census != codes).any(axis=0))[0]
    assert tuple(changed) == ls.HOT_SITES == names["cooled_sites"]
    assert np.array_equal(census[names["runs"]["all_n"]], codes[names["runs"]["all_n"]])
    # the cuts of world 2 and 3 fall inside panels 1, 0 and 1
    assert [b // 2048 for b, _ in sc.shares(4396, 2)[1:]] == [1] and [b // 2048 for b, _ in sc.shares(4396, 3)[1:]] == [0, 1]


def test_the_cooled_census_keeps_the_designed_lists(cooled):
    codes, names, ref, dev, hot, c = cooled
    bucket = c["bucket"]
    kept = {k: v for k, v in names["sized"].items() if v <= 142}
    assert sorted(set(kept.values())) == [1, 12, 13, 14, 15, 16, 17, 76, 77, 78, 140, 141, 142] and len(kept) == 3 * 16
    for (p, s), size in kept.items():
        assert int(bucket[p, s]) == size, (p, s)
    for (p, s), size in names["sized"].items():
        if size > 142:                                              # only the record of N is left at a cooled column
            assert int(bucket[p, s]) == (1 if p == 2 and ref[s] != 15 else 0), (p, s)
    over = bucket > ls.INLINE
    assert {(p, int(s)) for p, s in zip(*np.nonzero(over))} == {k for k, v in kept.items() if v > ls.INLINE}
    for (p, s), r in names["probes"].items():
        if (p, s) not in kept:
            continue
        assert c["diff"][r, s] and int((c["diff"][r] & over[p]).sum()) == (1 if names["sized"][(p, s)] > ls.INLINE else 0)
    for (r, chunk), count in names["slots"].items():
        assert int(c["per_chunk"][r, chunk]) == (120 if count == "N" else count), (r, chunk)
    for r, count in names["pieces"].items():
        assert int(c["per_range"][r, 2]) == count, r
    cold = sorted(int(c["length"][a] + c["length"][b]) for (a, b) in names["batches_cold"])
    assert cold == [127, 128, 129, 255, 256, 257, 511, 512, 513]
    assert {k: int(c["run_chunks"][r]) for k, r in names["runs"].items()} == {"three_chunks": 3, "four_chunks": 4,
                                                                             "four_with_partial": 4, "all_n": 33}
    assert ls.run_record_count(c["run_chunks"]) == 3
    assert [int(c["length"][r]) for r in names["near_root"]] == [0, 0, 0]     # now the root itself: empty lists


def test_wide_cut_set_has_65_ranges_and_the_trailing_marks(wide):
    codes, names, ref, dev, hot, c = wide
    k = len(names["keep"])
    assert codes.shape == (k + 3, 65664) and -(-65664 // 1024) == 65 and 65664 > 65536
    assert np.array_equal(ref, names["root"] >> 4) and int(hot.sum()) == 0
    rides_the_shared_path(codes, dev, hot, c, (2,))
    assert ls.run_record_count(c["run_chunks"]) >= 1
    added, per_range = names["added"], c["per_range"]
    assert added == {"beyond": k, "range_0": k + 1, "ranges_63_64": k + 2}
    sites = {key: np.nonzero(c["diff"][r])[0].tolist() for key, r in added.items()}
    assert len(sites["beyond"]) == 1 and sites["beyond"][0] >= 65536
    assert len(sites["range_0"]) == 5 and max(sites["range_0"]) == 1023 and int(per_range[added["range_0"], 1:].sum()) == 0
    assert [s // 1024 for s in sites["ranges_63_64"]] == [63, 64]
    assert [sc.range_marks(c["diff"][added["beyond"]], 65).tolist(), sc.range_marks(c["diff"][added["range_0"]], 65).tolist(),
            sc.range_marks(c["diff"][added["ranges_63_64"]], 65).tolist()] == [[0] * 65, [0] + [5] * 64, [0] * 64 + [1]]


def test_the_other_sets():
    diverse = sc.diverse_set()
    ref, dev, hot, c = view(diverse)
    assert diverse.shape == (600, 1000) and int(dev.sum()) > int(0.08 * 1000 * 512)            # past the gate
    assert 0.25 < c["diff"].mean() < 0.35
    for n in (2, 257, 300):
        codes = sc.small_set(n)
        ref, dev, hot, c = view(codes)
        assert codes.shape == (n, 300) and n <= 512
        rides_the_shared_path(codes, dev, hot, c, (2, 3))
        assert int(c["length"].sum()) > 0 and int((c["length"] == 0).sum()) > 0


@pytest.mark.parametrize("which", ("cut", "wide"))
def test_range_marks_restated(cut, wide, which):
    """mark g = the index of the first entry at or beyond site g * 1,024: the exclusive prefix of the per-range counts, and
    what 64 entries a round with a carried `next` find (range_marks_kernel's rule restated)"""
    codes, names, ref, dev, hot, c = cut if which == "cut" else wide
    n_ranges = c["per_range"].shape[1]
    prefix = np.cumsum(c["per_range"], axis=1) - c["per_range"]
    for r in range(len(codes)):
        marks = sc.range_marks(c["diff"][r], n_ranges)
        assert np.array_equal(marks, prefix[r]), r
        assert np.array_equal(sc.range_marks_by_rounds(c["diff"][r], n_ranges), marks), r
    if which == "cut":
        mid = names["mid"]
        assert sc.range_marks(c["diff"][mid[("ranges_0_and_4", None)]], 5).tolist() == [0, 5, 5, 5, 5]
        assert sc.range_marks(c["diff"][mid[("range_4_only", None)]], 5).tolist() == [0, 0, 0, 0, 0]
        assert sc.range_marks(c["diff"][mid[("range_0_only", None)]], 5).tolist() == [0, 9, 9, 9, 9]
        assert sc.range_marks(c["diff"][mid[("length", 0)]], 5).tolist() == [0, 0, 0, 0, 0]
        assert sc.range_marks(c["diff"][mid[("piece", 73)]], 5).tolist() == [0, 0, 0, 73, 73]


def test_the_oracle_agrees_with_the_per_site_table_on_feature_pairs(cut):
    codes, names = cut[0], cut[1]
    tables = ls.tally_tables()
    rng = np.random.default_rng(8)
    feat = np.array(sorted(names["features"]))
    pairs = [(int(a), int(b)) for a, b in zip(rng.choice(feat, 200), rng.choice(1100, 200)) if a != b]
    pairs += [(255, 256), (511, 512), (767, 768), (1023, 1024), (1099, 0)]
    for m in FAMILIES:
        for a, b in pairs:
            want = ls.table_tallies(tables[m], codes[a], codes[b])
            assert [int(x) for x in oracle.tallies(m, codes[a], codes[b])] == [int(x) for x in want], (m, a, b)
