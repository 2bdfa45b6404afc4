"""CPU: what tests/test_gpu_dense_census.py relies on, checked with the oracle and dst_plan_tiles — the designed records sit
where dense_census_cases says, every job shape has the partial tiles, the diagonal tile and the partial panel it is there
for at every tile height, neighbouring output slots hold different values (a kernel that stores a pair in a neighbour's
slot cannot pass on ties), and every instantiation of the table is named by a case."""
import math

import numpy as np
import pytest

import dense_census_cases as dc
import oracle
from helpers import CODES


def test_set_a_holds_every_code_and_the_designed_pairs():
    a, b = dc.codes_of("A"), dc.codes_of("B")
    assert a.shape == (771, 677) and b.shape == (100, 677)
    assert set(np.unique(a).tolist()) == set(CODES.tolist()) and set(np.unique(b).tolist()) == set(CODES.tolist())
    for codes, name, all_n, copy, trio in ((a, "A", dc.A_ALL_N, dc.A_COPY, dc.A_TRIO), (b, "B", dc.B_ALL_N, dc.B_COPY, dc.B_TRIO)):
        raw, jc, tn = (dc.oracle_distances(m, name, name) for m in ("raw", "jc69", "tn93"))
        others = np.arange(len(codes)) != all_n
        assert np.isnan(raw[all_n]).all() and np.isnan(tn[all_n]).all() and np.isnan(raw[:, all_n]).all()
        assert np.array_equal(codes[copy], codes[copy - 1])
        assert raw[copy - 1, copy] == 0 and jc[copy - 1, copy] == 0 and math.copysign(1, jc[copy - 1, copy]) == -1
        assert dc.oracle_distances("n_high", name, name)[copy - 1, copy] == 0
        x, y, z = trio
        assert math.isnan(jc[x, y]) and jc[x, z] == math.inf
        # and they are the exception: the rest of the set has finite distances (jc69: but for the trio's 20-site records)
        rest = others[:, None] & others[None, :] & ~np.eye(len(codes), dtype=bool)
        assert np.isfinite(raw[rest]).all() and (np.isfinite(jc[rest]).mean() > 0.95)
    # A: the all-N record is the first of the second panel, the copy its last record, the trio inside it
    assert dc.A_ALL_N == 512 and dc.A_COPY == len(a) - 1 and all(512 < r < 768 for r in dc.A_TRIO)
    assert len(a) - 768 == 3                    # the tn = 1 half of the second panel holds 3 records
    assert dc.chunks_of("A") == 6 and 677 - 5 * 128 == 37
    assert dc.chunks_of("C") == 17 and dc.codes_of("C").shape == (70, 2049)
    assert dc.codes_of("H").shape == (300, 2048) and dc.codes_of("HW").shape == (40, 65600)
    assert not dc.hot_is_wide("hybrid_square_whole") and dc.hot_is_wide("hybrid_wide_whole")


@pytest.mark.parametrize("measure,variant", dc.variants())
def test_every_job_shape_has_its_edges_at_every_tile_height(measure, variant):
    bm0, bn0 = dc.tile_of(measure, variant)
    assert bn0 == 512
    for name, shape in {**dc.SHAPES, "auto_split": dc.AUTO_SPLIT, **dc.HYBRID_SHAPES}.items():
        tiles, bm, bn = dc.plan(shape, measure, variant)
        assert (bm, bn) == (bm0, bn0)
        real = tiles[tiles[:, 0] != dc.FILLER].astype(np.int64)
        rb, re, square = shape["rb"], shape["re"], shape["square"]
        n_cols = len(dc.codes_of(shape["cols"]))
        # every pair of the job in exactly one tile, and no tile outside it
        cover = np.zeros((re - rb, n_cols), np.int32)
        for i0, j0 in real:
            assert rb <= i0 < re and (i0 - rb) % bm == 0 and j0 % bn == 0 and j0 < n_cols, (name, i0, j0)
            cover[i0 - rb:min(i0 + bm, re) - rb, j0:min(j0 + bn, n_cols)] += 1
        i, j = dc.pairs_of(shape)
        inside = np.zeros_like(cover, dtype=bool)
        inside[i - rb, j] = True
        assert (cover[inside] == 1).all(), (name, measure, variant)
        assert len(i) == int(inside.sum())
        if name not in dc.SHAPES:
            continue
        # the edges the shape is there for
        assert (re - rb) % bm != 0, (name, bm)                                  # a partial last row tile
        assert any(i0 + bm > re for i0, _ in real), (name, bm)
        assert n_cols % bn != 0                                                 # a partial last panel
        if square:
            assert any(j0 <= i0 < j0 + bn for i0, j0 in real), (name, bm)       # a tile on the diagonal
            assert name != "square_37_150" or rb % bm != 0, (name, bm)          # 37: i0 a multiple of no height
    # the panel edge on the diagonal: rows [500, 530) have tiles in both panels, the first panel's end at the diagonal
    tiles, bm, _ = dc.plan(dc.SHAPES["square_500_530"], measure, variant)
    real = tiles[tiles[:, 0] != dc.FILLER].astype(np.int64)
    assert {int(j0) for _, j0 in real} == {0, 512} and all(i0 < 511 for i0, j0 in real if j0 == 0)


@pytest.mark.parametrize("measure", dc.F64)
def test_the_reference_and_the_exact_value_agree_off_the_singular_pairs(measure):
    """30 % divergence puts k80's 2P + Q around 1: where a logarithm's argument is exactly 0 the exact value is +inf and
    the reference's f64 formula gives a rounding residue.  Those pairs are few, and everywhere else the two agree on NaN,
    inf and 0 — what check_f64 asserts before it compares values."""
    for name, shape in {**dc.SHAPES, "auto_split": dc.AUTO_SPLIT, **dc.HYBRID_SHAPES}.items():
        x = dc.want_exact(measure, shape).value.astype(np.float64)
        want = dc.want_distances(measure, shape)
        sing = dc.singular(measure, shape)
        differ = (np.isnan(x) != np.isnan(want)) | (np.isinf(x) != np.isinf(want)) | ((x == 0) != (want == 0))
        assert not (differ & ~sing).any(), (measure, name)
        assert sing.mean() <= 0.01, (measure, name, sing.mean())
        if shape["rows"] in ("A", "B"):        # most pairs have a finite distance: the bars have something to hold
            assert np.isfinite(want).mean() >= 0.9, (measure, name, np.isfinite(want).mean())


def test_forced_and_automatic_split_factors():
    shape = dc.SHAPES["square_37_150"]
    assert [dc.forced_ksplit(k, shape) for k in dc.FORCED] == [2, 4, 6]
    # 4 parts of 6 chunks: 1, 2, 1 and 2 chunks (c_begin = floor(6 part / 4))
    cuts = [6 * p // 4 for p in range(5)]
    assert [b - a for a, b in zip(cuts, cuts[1:])] == [1, 2, 1, 2]
    for measure in dc.ALL:
        for v in (0, dc.tallest_variant(measure)):
            tiles, _, _ = dc.plan(dc.AUTO_SPLIT, measure, v)
            assert dc.automatic_ksplit(len(tiles), dc.chunks_of("C")) == 2, (measure, v)
        for name in dc.SHAPES:            # set A's 6 chunks: no automatic split
            tiles, _, _ = dc.plan(dc.SHAPES[name], measure, 0)
            assert dc.automatic_ksplit(len(tiles), dc.chunks_of("A")) == 1


@pytest.mark.parametrize("measure", ("n_high", "raw", "k80", "tn93"))
def test_neighbouring_slots_differ(measure):
    """The oracle's tally vector of pair (i, j) of A against those of (i + 1, j), (i, j + 1), (i, j + 256) (the lane's
    other column) and (i + bm / 2, j) (the same slot of the other epilogue pass) for every tile height: at most 5 % of the
    pairs equal any one of them.  A cap on what the data may hide, not a tolerance of the kernel."""
    tl = dc.oracle_tallies(measure, "A", "A")
    n = len(tl)
    heights = sorted({dc.tile_of(m, v)[0] for m, v in dc.variants()})
    assert heights == [8, 12, 16, 24, 32]
    upper = np.triu(np.ones((n, n), bool), 1)
    for di, dj in [(1, 0), (0, 1), (0, 256)] + [(bm // 2, 0) for bm in heights]:
        both = upper[:n - di, :n - dj] & upper[di:, dj:]
        same = (tl[:n - di, :n - dj] == tl[di:, dj:]).all(axis=2) & both
        share = same.sum() / upper.sum()
        print(f"{measure}: pairs equal to their neighbour at (+{di}, +{dj}): {100 * share:.2f} %")
        assert share <= dc.NEIGHBOUR_TIE_CAP, (measure, di, dj, share)
    first = tl[..., 0][upper]
    print(f"{measure}: {len(np.unique(tl[upper], axis=0))} distinct tally vectors, first tally {first.min()} to {first.max()}")


def test_the_table_has_fifty_entries_each_named_by_a_case():
    table = dc.build_table()
    assert len(table) == dc.EXPECTED_INSTANTIATIONS, sorted(table)
    per_family = {fam: sorted({bm for f, bm, _ in table if f == fam}) for fam in range(4)}
    assert all(len(v) == (2 if fam == 2 else 3) for fam, v in per_family.items()), per_family
    named = {}
    for measure, variant in dc.variants():
        for key, cases in dc.cases_naming(measure, variant).items():
            named.setdefault(key, []).extend(cases)
    assert set(named) == table, (sorted(table - set(named)), sorted(set(named) - table))
    assert all(named[key] for key in table)
    # a variant out of range is variant 0 (pick_variant)
    for measure in dc.ALL:
        assert dc.tile_of(measure, -1) == dc.tile_of(measure, 0) == dc.tile_of(measure, dc.variant_count(measure))
    # the oracle's tallies of a pair are the reference's, whichever way they are fetched
    a = dc.codes_of("A")
    for measure in ("n_high", "raw", "k80", "tn93"):
        for i, j in ((0, 1), (511, 512), (769, 770), (600, 601)):
            assert list(dc.oracle_tallies(measure, "A", "A")[i, j]) == list(oracle.tallies(measure, a[i], a[j]))
