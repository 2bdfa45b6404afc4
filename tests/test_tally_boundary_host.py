"""CPU: the designed alignments of tally_boundary_cases.py hold the saturated patterns test_gpu_tally_boundary.py relies
on — asserted on the oracle alone, so that the GPU test cannot lose its edge unnoticed — and the exported launch planner
tells the narrow form from the wide one.

Tally slots (oracle.tallies): n_high {d}; raw {n differences, d compared}; k80 {count_L, transitions, transversions};
tn93 {count_L, count_d, count_P1, count_P2}.  The narrow form packs slots 0/1 (and tn93's 2/3) as low + 65536 * high."""
import os

import numpy as np
import pytest

import distance_amd as da
import oracle
import tally_boundary_cases as tb

THREADS = min(16, len(os.sched_getaffinity(0)))
FAMILIES = ("n_high", "raw", "k80", "tn93")


def named_tallies(codes, names, cols=None):
    """{family: tallies (k, k, width)} of the named records and three of the majority among each other, and their labels"""
    idx = tb.extremes(names) + names["majority"][:3]
    sub = codes[idx] if cols is None else np.ascontiguousarray(codes[idx][:, cols])
    label = {v: k for k, v in names.items() if k in tb.PLACES}
    labels = [label.get(r, "majority_%d" % r) for r in idx]
    return {m: oracle.tallies_rect(m, sub, sub, threads=THREADS) for m in FAMILIES}, labels


def has(t, **slots):
    """is there a pair of two different records whose tallies in the given slots (s0=.., s1=..) are exactly these?"""
    ok = ~np.eye(t.shape[0], dtype=bool)
    for key, v in slots.items():
        ok &= t[:, :, int(key[1:])] == v
    return bool(ok.any())


def of(t, labels, a, b):
    return [int(x) for x in t[labels.index(a), labels.index(b)]]


@pytest.mark.parametrize("L", tb.WIDTHS)
def test_the_plain_set_holds_every_saturated_pattern(L):
    codes, names = tb.boundary_alignment(L, "plain")
    assert codes.shape == (tb.N_RECORDS, L)
    t, lab = named_tallies(codes, names)
    # every tally slot of every family reaches L itself: 0xFFFF at 65,535 sites, past 16 bits from 65,536 on
    for m in FAMILIES:
        for s in range(oracle.N_TALLIES[m]):
            assert has(t[m], **{"s%d" % s: L}), (m, s)
    # the packed pairs of slots (low, high).  Both all ones:
    assert has(t["raw"], s0=L, s1=L)        # ts_all against tv_all: every site compared, every site different
    assert has(t["k80"], s0=L, s1=L)        # pur against pur_ts: every site a transition
    assert has(t["tn93"], s0=L, s1=L)
    # tn93 2/3 (count_P1, count_P2) cannot both be L: a site is a purine transition or a pyrimidine one, P1 + P2 <= count_d <= L
    # low = 0, high = L: the low half's additions and subtractions cancel exactly while the high half is all ones
    assert of(t["raw"], lab, "ts_all", "ts_all_copy") == [0, L]     # both differ from the plurality at every site, equal to each other
    assert has(t["tn93"], s2=0, s3=L)       # pyr against pyr_ts
    # k80 0/1 and tn93 0/1 cannot have low = 0 with high = L: transitions <= count_L and count_d <= count_L
    # low = L, high = 0:
    assert of(t["k80"], lab, "ts_all", "ts_all_copy")[:2] == [L, 0]
    assert of(t["tn93"], lab, "ts_all", "ts_all_copy")[:2] == [L, 0]
    assert has(t["tn93"], s2=L, s3=0)       # pur against pur_ts
    # raw cannot have low = L with high = 0: n <= d, a difference is a compared site
    # k80's third tally has a word of its own (never split): L and 0 next to a saturated first word
    assert of(t["k80"], lab, "ts_all", "tv_all") == [L, 0, L]
    assert of(t["k80"], lab, "pur", "pur_ts") == [L, L, 0]
    assert of(t["tn93"], lab, "pur", "pur_ts") == [L, L, L, 0]
    assert of(t["tn93"], lab, "pyr", "pyr_ts") == [L, L, 0, L]
    assert of(t["tn93"], lab, "ts_all", "tv_all") == [L, L, 0, 0]
    assert of(t["n_high"], lab, "ts_all", "tv_all") == [L]
    # bit 15 alone, and what is left of L beside it
    assert of(t["raw"], lab, "first_half", "ts_all") == [tb.HALF, tb.HALF]
    assert of(t["raw"], lab, "second_half", "ts_all") == [L - tb.HALF, L - tb.HALF]
    assert of(t["raw"], lab, "first_half", "root") == [0, tb.HALF]
    assert of(t["tn93"], lab, "first_half", "ts_all")[:2] == [tb.HALF, tb.HALF]
    assert of(t["k80"], lab, "second_half", "tv_all") == [L - tb.HALF, 0, L - tb.HALF]
    assert of(t["raw"], lab, "first_half", "second_half") == [0, 0]
    # nothing at all, and exactly one site
    for m in FAMILIES:
        row = t[m][lab.index("all_n")]
        assert not row.any(), m
    assert of(t["raw"], lab, "one_site", "root") == [1, 1]
    assert of(t["raw"], lab, "last_site_only", "root") == [1, 1]
    assert of(t["raw"], lab, "last_site_only", "second_half") == [1, 1]
    assert of(t["raw"], lab, "one_site", "last_site_only") == [0, 0]
    # on which side of the switch this width lies
    top = max(int(t[m].max()) for m in FAMILIES)
    assert top == L and (top > 0xFFFF) == tb.wide_of(L) and (L != 65535 or top == 0xFFFF)


@pytest.mark.parametrize("L", tb.WIDTHS)
@pytest.mark.parametrize("kind", tb.KINDS)
def test_the_sets_meet_the_engine_rules_they_were_laid_out_for(L, kind):
    """the counts of tally_boundary_cases' docstring: cold sites below the 5 % of the hot rule, the mean deviation below
    the 8 % of the fused preparation, the names in different thirds of the triangle"""
    codes, names = tb.boundary_alignment(L, kind)
    n = len(codes)
    dev = tb.deviants(codes)
    assert dev.sum() <= 0.08 * n * L
    hot = dev * 1000 > n * 50
    if kind == "hot":
        cols = names["hot_columns"]
        assert len(cols) == L // 2 and np.array_equal(np.nonzero(hot)[0], cols)       # as many as the hybrid path admits
    elif kind == "plain":
        assert not hot.any()
    b = da.partition_square(n, 3)
    part = lambda r: int(np.searchsorted(b, r, side="right")) - 1                    # noqa: E731
    assert {part(names[k]) for k in ("ts_all", "ts_all_copy", "tv_all")} == {0, 1, 2}
    if kind == "runs":
        nch = -(-L // 128)
        padded = np.full((n, nch * 128), tb.N, np.uint8)
        padded[:, :L] = codes
        whole = (padded == tb.N).reshape(n, nch, 128).all(axis=2).sum(axis=1)
        for r in names["runs"]:
            assert whole[r] >= 4, r                                                  # kRunMin whole chunks of N
            assert (codes[r] != tb.N).sum() > 20_000                                 # and a body outside the runs
        assert (whole >= 4).sum() <= n // 3                                          # all of them fit the run-record budget


@pytest.mark.parametrize("L", tb.WIDTHS)
def test_the_hot_columns_alone_carry_half_the_alignment(L):
    """kind "hot": the tallies of the named records restricted to the hot columns.  The hybrid path hands a launch to the
    dense kernels once more than half of the sites are hot, so floor(L / 2) columns is the most a hot tally can be: 32,767
    (0x7FFF) for both narrow widths — bit 15 of a 16-bit hot tally is out of reach by that rule — and 32,768 from 65,536
    sites on."""
    codes, names = tb.boundary_alignment(L, "hot")
    cols = names["hot_columns"]
    t, lab = named_tallies(codes, names, cols)
    H = L // 2
    assert of(t["raw"], lab, "ts_all", "tv_all") == [H, H]
    assert of(t["tn93"], lab, "pur", "pur_ts") == [H, H, H, 0]
    assert of(t["k80"], lab, "ts_all", "tv_all") == [H, 0, H]
    assert (H >= tb.HALF) == tb.wide_of(L)
    # and the clade records differ from the majority there
    clade = oracle.tallies("raw", codes[names["clade"][0]][cols], codes[names["root"]][cols])
    assert list(clade) == [H, H]


def test_the_planner_tells_narrow_from_wide():
    assert [tb.wide_of(L) for L in tb.WIDTHS] == [False, False, True, True]
    for L in (65535, 65536):
        wide = tb.wide_of(L)
        pairs = tb.N_RECORDS * (tb.N_RECORDS - 1) // 2
        for m in ("n", "n_high", "raw", "jc69", "k80", "tn93"):
            for kind in (da.OUT_DISTANCE, da.OUT_TALLY):
                d = da.plan_consensus_launch(m, kind, wide, True, tb.N_RECORDS, tb.N_RECORDS, pairs, 0.1, 15.0)
                assert d["wide"] == wide and d["path"] == "consensus", (L, m, kind)
        # the plan differs: tn93's distance output runs without roles in the narrow form, with one event wave in the wide one
        d = da.plan_consensus_launch("tn93", da.OUT_DISTANCE, wide, True, 40_000, 40_000, 40_000 * 39_999 // 2, 0.1, 15.0)
        assert d["event_waves"] == (1 if wide else 8), (L, d)
        # the 16-bit output exists in the narrow form only
        if wide:
            with pytest.raises(da.DistanceError) as e:
                da.plan_consensus_launch("raw", da.OUT_TALLY16, wide, True, 100, 100, 4950, 0.1, 15.0)
            assert e.value.status == 1
        else:
            assert da.plan_consensus_launch("raw", da.OUT_TALLY16, wide, True, 100, 100, 4950, 0.1, 15.0)["wide"] is False
