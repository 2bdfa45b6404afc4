"""CPU: the designed sets of list_structure_cases.py hold every slot, piece, bucket, batch and run-record size that
test_gpu_list_structure.py relies on — counted from the code matrix alone, so that a retune of a constant or an edit of the
generator cannot move the GPU test off its boundaries unnoticed — and the design is tied to the oracle.

The constants restated here are the engine's (dst_internal.h, dst_consensus.hip): kSlotEntries 7, kBucketWalk 8 and 64 a
round, kInlineEvents 15 / kInlineOverflowing 13 with 128 overflow entries a round, kEventLanes 128 / 256 / 512, kRunMin 4
and n / 3, the 512-record sample with floor(k n / 512), kHotPermille 50 and the fused preparation's 8 % gate."""
import numpy as np
import pytest

import list_structure_cases as ls
import oracle

FAMILIES = ("n_high", "raw", "k80", "tn93")


@pytest.fixture(scope="module")
def design():
    codes, names = ls.census_alignment()
    ref, dev, hot = ls.sampled_reference(codes)
    return codes, names, ref, dev, hot, ls.census(codes, ref)


def test_the_shape_is_two_full_panels_and_one_of_300_records(design):
    codes = design[0]
    assert codes.shape == (4396, 4200) == (ls.N_RECORDS, ls.LENGTH)
    assert [len(codes[p * 2048:(p + 1) * 2048]) for p in range(3)] == [2048, 2048, 300] == list(ls.PANEL_SIZE)
    assert -(-4200 // 128) == 33 and 4200 - 32 * 128 == 104 and -(-4200 // 1024) == 5


def test_the_sample_takes_the_root_and_the_gates_hold(design):
    codes, names, ref, dev, hot, _ = design
    # the sampling rule restated: record floor(k n / 512), and the engine's shift form of it (sample_record)
    k, n = np.arange(512, dtype=np.int64), ls.N_RECORDS
    assert np.array_equal(ls.sampled_records(n), k * (n >> 9) + ((k * (n & 511)) >> 9))
    per_panel = [int(((ls.sampled_records(n) // 2048) == p).sum()) for p in range(3)]
    assert per_panel == [239, 239, 34]
    # the plurality (strict > over A, G, C, T, N class) is the root's class at every site
    assert np.array_equal(ref, names["root"] >> 4)
    assert int((ref == 15).sum()) == int((np.arange(4200) % 16 == 5).sum()) + sum(c == 4 and s % 16 != 5 for s, _, c in ls.SIZED_SITES)
    # the fused preparation's gate: the sampled records deviate at no more than 8 % of the sites
    assert int(dev.sum()) <= int(0.08 * 4200 * 512)
    # hot: more than 25.6 of the 512 sampled records deviate.  The panel-wide buckets are, everything else is not
    assert tuple(np.nonzero(hot)[0]) == names["hot_sites"] and len(names["hot_sites"]) == 6
    assert 2 * int(hot.sum()) <= 4200
    sized = names["sized"]
    assert {v for (p, s), v in sized.items() if hot[s]} == {2047, 2048, 299, 300}
    assert max(int(dev[s]) for (p, s), v in sized.items() if v <= 142) <= 19
    assert int(dev[~hot].max()) <= 19
    # background records make no entry: N, - and ? all occur at the N-class sites of records without a feature
    plain = [r for r in range(200, 2040) if r not in set(names["features"])][:30]
    ncls = np.nonzero(ref == 15)[0]
    assert {int(x) for x in np.unique(codes[plain][:, ncls])} >= {240, 244, 242}


def test_bucket_sizes_sit_where_the_design_says(design):
    codes, names, ref, dev, hot, c = design
    sized, bucket = names["sized"], c["bucket"]
    for (p, s), size in sized.items():
        assert int(bucket[p, s]) == size, (p, s, size)
        assert s < 1024
    for p in range(3):
        full = ls.PANEL_SIZE[p]
        want = sorted([1, 12, 13, 14, 15, 16, 17, 76, 77, 78, 140, 141, 142, full - 1, full] + [15, 16, 17])
        assert sorted(v for (q, s), v in sized.items() if q == p) == want
        # in-panel record 0 and the panel's last are members (size 1: the last alone)
        first, last = ls.PANEL_START[p], ls.PANEL_START[p] + full - 1
        for (q, s), size in sized.items():
            if q == p:
                assert c["diff"][last, s] and (size == 1 or c["diff"][first, s]), (p, s)
    # either side of kInlineEvents, and the overflow beyond kInlineOverflowing at 64 / 128 and one either side
    assert {15, 16} <= set(sized.values()) and 16 > ls.INLINE >= 15
    assert {v - ls.INLINE_OVER for v in sized.values() if v > ls.INLINE} >= {63, 64, 65, 127, 128, 129}
    # three sites carry 15, 16 and 17 in all three panels at once
    for size in (15, 16, 17):
        assert any(all(sized.get((p, s)) == size for p in range(3)) for s in range(1024))
    # the reference class runs round-robin over the sites of 140 and more: each of the five classes three times
    big = [int(ref[s]) for (p, s), v in sized.items() if v >= 140]
    assert sorted(big) == sorted(3 * list(ls.CLASS_NIBBLE))
    # a probe of panel 0 for every site of 12 and more of panels 1 and 2: its only entry in an overflowing bucket of that
    # column panel, its batch neighbour without one
    over = bucket > ls.INLINE
    assert {(p, int(s)) for p, s in zip(*np.nonzero(over))} == {k for k, v in sized.items() if v > ls.INLINE}   # and no other overflows
    assert len(names["probes"]) == 28
    for (p, s), r in names["probes"].items():
        assert r < 2048 and r % 2 == 0 and c["diff"][r, s] and sized[(p, s)] >= 12
        assert int((c["diff"][r] & over[p]).sum()) == (1 if sized[(p, s)] > ls.INLINE else 0), (p, s, r)
        assert int((c["diff"][r + 1] & over[p]).sum()) == 0
    # the 11-bit record-in-panel field: 0 and 2,047 are both in buckets that overflow and in buckets that do not
    assert c["diff"][2047, [s for (p, s), v in sized.items() if p == 0 and v == 1][0]]


def test_slots_hold_the_named_differences(design):
    codes, names, ref, dev, hot, c = design
    seen = set()
    for (r, chunk), count in names["slots"].items():
        assert 8 <= chunk <= 15 and 1 <= r % 2048 <= 8
        if count == "N":
            assert np.all(codes[r, chunk * 128:(chunk + 1) * 128] >> 4 == 15) and c["run_chunks"][r] == 1
            assert int(c["per_chunk"][r, chunk]) == 120          # the eight N-class sites of the chunk make no entry
        else:
            assert int(c["per_chunk"][r, chunk]) == count, (r, chunk)
            assert c["run_chunks"][r] == 0
        seen.add(count)
        # nothing else of the record in chunks 8-15
        assert int(c["per_chunk"][r, 8:16].sum()) == int(c["per_chunk"][r, chunk])
    assert seen == {1, 6, 7, 8, 9, 127, 128, "N"} and ls.SLOT_ENTRIES == 7
    assert len(names["slots"]) == 24
    # the partial last chunk: 104 sites, all of them entries of the record that is N there
    r = names["runs"]["four_with_partial"]
    assert int(c["per_chunk"][r, 32]) == 104 - int((ref[4096:] == 15).sum())


def test_pieces_hold_the_named_entries(design):
    codes, names, ref, dev, hot, c = design
    for r, count in names["pieces"].items():
        assert 9 <= r % 2048 <= 16 and int(c["per_range"][r, 2]) == count, r
        assert int(c["per_range"][r, 1]) == int(c["per_range"][r, 3]) == int(c["per_range"][r, 4]) == 0
    assert sorted(set(names["pieces"].values())) == [7, 8, 9, 10, 71, 72, 73, 137]
    # 8 walked by the thread, then rounds of 64: one short of, at and one past the walk, one round and two rounds
    w = ls.BUCKET_WALK
    assert {w - 1, w, w + 1, w + 63, w + 64, w + 65, w + 129} <= set(names["pieces"].values())
    assert len(names["pieces"]) == 24


def test_batches_sum_to_the_pipeline_widths(design):
    codes, names, ref, dev, hot, c = design
    cold = (c["diff"] & ~hot[None, :]).sum(axis=1)
    for key, length, first in (("batches", c["length"], 32), ("batches_cold", cold, 50)):
        got = [int(length[a] + length[b]) for (a, b) in sorted(names[key])]
        assert got == [127, 128, 129, 255, 256, 257, 511, 512, 513], key
        assert sorted(names[key]) == [(first + 2 * i, first + 2 * i + 1) for i in range(9)]
        for (a, b), total in names[key].items():
            assert names[key][(a, b)] == total and int(length[a]) == total // 2
    # their own entries lie in sites 3,072-4,095; the rest are the two panel-wide buckets of panel 0
    for pair in list(names["batches"]) + list(names["batches_cold"]):
        for r in pair:
            assert int(c["per_range"][r, 0]) == 2 and int(c["per_range"][r, 1] + c["per_range"][r, 2] + c["per_range"][r, 4]) == 0
    # with tiles of 8 rows from row 0 the named rows are batches of a whole-triangle launch
    sums = ls.batch_sums(c["length"], 0, 4396, 8, 2047)
    assert {64 * ew + d for ew in (2, 4, 8) for d in (-1, 0, 1)} <= set(sums)
    assert {64 * ew + d for ew in (2, 4, 8) for d in (-1, 0, 1)} <= set(ls.batch_sums(cold, 0, 4396, 8, 2047))
    # a launch from row 33 pairs the rows the other way
    assert ls.batch_sums(c["length"], 33, 60, 8)[:3] == [64 + 64, 64 + 64, 65 + 127]
    assert ls.batch_sums(c["length"], 32, 33, 8) == [63] and len(ls.batch_sums(c["length"], 0, 45, 8)) == 23      # single-row batches


def test_run_chunks_and_ends(design):
    codes, names, ref, dev, hot, c = design
    runs = names["runs"]
    assert {k: int(c["run_chunks"][r]) for k, r in runs.items()} == {"three_chunks": 3, "four_chunks": 4, "four_with_partial": 4,
                                                                    "all_n": 33}
    assert np.all(codes[runs["four_with_partial"], 4096:] >> 4 == 15) and np.all(codes[runs["all_n"]] >> 4 == 15)
    assert ls.run_record_count(c["run_chunks"]) == 3 == int((c["run_chunks"] >= ls.RUN_MIN).sum())
    assert [int(c["length"][r]) for r in names["near_root"]] == [1, 1, 1]
    assert int(c["length"].min()) == 1           # no empty list here: the panel-wide buckets hold every record


def test_every_nibble_pair_meets_at_every_reference_class(design):
    """14 x 14 x 5 = 980 triples (row nibble, column nibble, reference class), both nibbles different from the reference's:
    each occurs at some site of some pair of different records"""
    codes, names, ref, dev, hot, c = design
    nib = codes >> 4
    seen = set()
    for s in sorted({s for (_, s) in names["sized"]}):
        cnt = np.bincount(nib[c["diff"][:, s], s], minlength=16)
        cls = ls.CLASS_NIBBLE.index(int(ref[s]))
        for a in range(1, 16):
            for b in range(1, 16):
                if cnt[a] and cnt[b] and (a != b or cnt[a] >= 2):
                    seen.add((a, b, cls))
    assert len(seen) == 980
    assert all(a != ls.CLASS_NIBBLE[k] and b != ls.CLASS_NIBBLE[k] for a, b, k in seen)


def test_the_oracle_agrees_with_the_per_site_table_on_feature_pairs(design):
    codes, names = design[0], design[1]
    tables = ls.tally_tables()
    rng = np.random.default_rng(7)
    feat = np.array(names["features"])
    pairs = [(int(a), int(b)) for a, b in zip(rng.choice(feat, 200), rng.choice(feat, 200)) if a != b]
    pairs += [(names["runs"]["all_n"], 0), (0, 2047), (32, 33), (4395, 4096)]
    for m in FAMILIES:
        for a, b in pairs:
            want = ls.table_tallies(tables[m], codes[a], codes[b])
            assert [int(x) for x in oracle.tallies(m, codes[a], codes[b])] == [int(x) for x in want], (m, a, b)


def test_the_partner_set_probes_panel_0(design):
    codes, names, ref, dev, hot, c = design
    partner = ls.partner_alignment()
    assert partner.shape == (130, 4200)
    pdiff = (partner >> 4) != ref[None, :]
    sized_at = {s for (_, s) in names["sized"]}
    over = c["bucket"] > ls.INLINE
    shared = set()
    for i in range(130):
        mine = set(np.nonzero(pdiff[i])[0].tolist())
        assert mine & sized_at
        for p in range(3):
            k = int((pdiff[i] & over[p]).sum())
            assert k <= 1
            if k and p == 0:
                s = int(np.nonzero(pdiff[i] & over[0])[0][0])
                shared.add(int(c["bucket"][0, s]) - ls.INLINE_OVER)
    assert shared >= {63, 64, 65, 127, 128, 129}


@pytest.mark.parametrize("n_run", ls.RUN_TABLE_N_RUN)
def test_run_table_sets_make_the_named_run_records(n_run):
    codes = ls.run_table_alignment(n_run)
    assert codes.shape == (700, 1280) and 700 // 3 == 233
    ref, dev, hot = ls.sampled_reference(codes)
    assert int(dev.sum()) <= int(0.08 * 1280 * 512)              # the fused preparation keeps its lists
    c = ls.census(codes, ref)
    assert int((c["run_chunks"] >= 4).sum()) == n_run and int(c["run_chunks"].max()) == 4
    assert ls.run_record_count(c["run_chunks"]) == (n_run if n_run <= 233 else 0)
    assert int((c["length"] == 0).sum()) > 100                     # records equal to the root: empty lists
    if n_run >= 32:
        masks = (codes[:n_run].reshape(n_run, 10, 128) >> 4 == 15).all(axis=2)
        overlap = masks.astype(int) @ masks.T.astype(int)
        assert set(np.unique(overlap)) == {0, 1, 2, 3, 4}         # the masks overlap partly


@pytest.mark.parametrize("L,words", [(32768, 8), (32896, 9)])
def test_long_run_table_sets_fill_eight_and_nine_mask_words(L, words):
    codes = ls.run_table_alignment(40, n=300, L=L, n_class_every=16, seed=L)
    nch = -(-L // 128)
    assert -(-nch // 32) == words
    c = ls.census(codes)
    assert ls.run_record_count(c["run_chunks"]) == 40
    masks = (codes[:40].reshape(40, nch, 128) >> 4 == 15).all(axis=2)
    assert masks[:, nch - 1].any() and masks[:, 0].any()
    assert len({int(k) // 32 for k in np.nonzero(masks.any(axis=0))[0]}) == words      # every mask word is in use
    ref, dev, hot = ls.sampled_reference(codes)
    assert int(dev.sum()) <= int(0.08 * L * 300)


def test_the_wide_form_keeps_the_feature_records(design):
    codes, names = design[0], design[1]
    wide, keep = ls.wide_form(codes, names)
    assert wide.shape[1] == 65664 == 513 * 128 and set(names["features"]) <= set(keep) and len(keep) <= 2048
    assert len(keep) - len(names["features"]) >= 560
    assert np.array_equal(wide[:, :4200], codes[keep]) and np.all(wide[:, 4200:] == ls.A)
    ref, dev, hot = ls.sampled_reference(wide)
    assert int(dev.sum()) <= int(0.08 * 65664 * 512)
    c = ls.census(wide, ref)
    assert {1, 6, 7, 8, 9, 127, 128} <= set(np.unique(c["per_chunk"])) and {7, 8, 9, 10, 71, 72, 73, 137} <= set(np.unique(c["per_range"]))
    assert ls.run_record_count(c["run_chunks"]) >= 1
