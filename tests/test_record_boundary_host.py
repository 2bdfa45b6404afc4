"""No GPU: the designed set of record_boundary_cases.py held to the oracle, not to itself, and the counts the GPU tests
rely on (test_gpu_record_boundary.py, test_gpu_record_boundary_windows.py, test_gpu_cli_record_boundary.py).

On the picked rows the closed forms (n, comparable, transitions, transversions, base counts) are the oracle's tallies of
the code bytes, the Walsh-Hadamard histogram and the bit-flip links are brute force over those rows, and the greedy slab
cut restated loop by loop gives the slabs the GPU tests ask for."""
import numpy as np
import pytest

import oracle
import record_boundary_cases as rbc
from record_boundary_cases import FIRST_ROW_PAST_2_32, N_RECORDS, POP, TWO32, canon, row_start

MEASURES = ("n", "n_high", "raw", "jc69", "k80", "tn93")
PAST_2_32_CUT = (33_594_324, 129, 91_504)   # (the bound, its slabs, the last slab's first row)


@pytest.fixture(scope="module")
def rs():
    return rbc.record_set()


def test_the_set_crosses_both_boundaries(rs):
    n = rs.n
    assert n == N_RECORDS == 92_700 and n * (n - 1) // 2 == 4_296_598_650 > TWO32
    assert row_start(n, 65_536) == 3_927_670_784
    assert row_start(n, FIRST_ROW_PAST_2_32 - 1) < TWO32 <= row_start(n, FIRST_ROW_PAST_2_32) and FIRST_ROW_PAST_2_32 == 90_894
    assert len(np.unique(rs.words)) == n and int(rs.words.max()) < 1 << rbc.BITS
    assert not np.array_equal(rs.words, np.sort(rs.words))   # input order is not word order
    assert rs.codes.shape == (n, 40) and set(np.unique(rs.codes)) == {rbc.A, rbc.G, rbc.C, rbc.N}
    for fixed in rbc.FIXED_ROWS:
        assert fixed in rs.picked
    assert 290 <= len(rs.picked) <= 300 and np.array_equal(rs.picked, np.unique(rs.picked))
    ids = rs.ids()
    assert len(set(ids)) == n and len({len(i) for i in ids}) >= 8   # ids of mixed length


def test_closed_forms_are_the_oracles_tallies(rs):
    rng = np.random.default_rng(7)
    for r in rs.picked:
        cols = rng.choice(rs.n, 200, replace=False)
        cols[:4] = (r, (r + 1) % rs.n, (r + 2) % rs.n, 65_536)   # itself, both other residues of r % 3
        rows = np.full(len(cols), r)
        for m in MEASURES:
            got = oracle.tallies_rect(m, rs.codes[r:r + 1], rs.codes[cols])[0]
            assert np.array_equal(got, rs.tallies(m, rows, cols).astype(np.uint64)), (int(r), m)
    some = np.concatenate([rs.picked, rng.choice(rs.n, 200, replace=False)])
    assert np.array_equal(oracle.count_bases_matrix(rs.codes[some]), rs.base_counts()[some].astype(np.uint64))
    # raw: the numpy quotient is the oracle's value to the bit, the three denominators interleave
    r = int(rs.picked[5])
    cols = rng.choice(rs.n, 200, replace=False)
    want = oracle.all_pairs_rect("raw", rs.codes[r:r + 1], rs.codes[cols])[0]
    assert np.array_equal(want.view(np.uint64), rs.values("raw", np.full(200, r), cols).view(np.uint64))
    assert 1 / 40 < 1 / 39 < 1 / 38 < 2 / 40 < 2 / 39 < 2 / 38 < 3 / 40


def test_histogram_and_sums_against_brute_force_rows(rs):
    brute, sums = np.zeros(rbc.BITS + 1, np.int64), rs.sums()
    for r in rs.picked:
        d = POP[rs.words[r] ^ rs.words]
        brute += np.bincount(d, minlength=rbc.BITS + 1)
        assert int(d.sum()) == int(sums[r]), int(r)
    counts = rbc.xor_counts(rs.words[rs.picked], rs.words)   # the same transform, restricted to the picked rows
    assert np.array_equal(np.array([int(counts[POP == d].sum()) for d in range(rbc.BITS + 1)]), brute)
    hist = rs.histogram()
    assert int(hist.sum()) == rs.n * (rs.n - 1) // 2 and hist[0] == 0
    assert int((hist * np.arange(rbc.BITS + 1, dtype=np.uint64)).sum()) * 2 == int(sums.sum())
    i, j, d = rs.links_within(2)
    assert hist[1] == (d == 1).sum() and hist[2] == (d == 2).sum()


def test_links_against_brute_force_rows_and_their_counts(rs):
    n = rs.n
    i, j, d = rs.links_within(2)
    assert (i < j).all() and (np.diff(canon(n, i, j)) > 0).all()   # canonical order, every pair once
    assert np.array_equal(d, rs.values("n", i, j))
    for r in rs.picked:
        row = POP[rs.words[r] ^ rs.words].astype(np.int64)
        row[r] = 99
        for radius in (1, 2):
            want = np.nonzero(row <= radius)[0]
            mine = np.sort(np.concatenate([j[(i == r) & (d <= radius)], i[(j == r) & (d <= radius)]]))
            assert np.array_equal(mine, want), (int(r), radius)
    # the counts the GPU tests rely on
    assert (d == 1).sum() == 81_846 and len(d) == 860_980
    at = canon(n, i, j)
    assert (at >= TWO32).sum() == 346 and ((at >= TWO32) & (d == 1)).sum() == 30
    assert (i >= 65_536).sum() == 74_033 and (j >= 65_536).sum() == 430_058
    assert ((i >= 65_536) & (d == 1)).sum() > 0 and (i >= FIRST_ROW_PAST_2_32).sum() > 0
    # raw: a threshold between 1/38 and 2/40 links the distance-1 pairs alone; one between 2/40 and 2/39 adds the
    # distance-2 pairs whose two records have all 40 sites
    full = (d == 2) & (rs.comparable(i, j) == 40)
    assert 0 < full.sum() < (d == 2).sum()
    raw = rs.values("raw", i, j)
    assert np.array_equal(raw <= 0.04, d == 1) and np.array_equal(raw <= 0.0505, (d == 1) | full)
    assert 1 / 38 < 0.04 < 2 / 40 < 0.0505 < 2 / 39


def test_clusters_and_mst_counts(rs):
    lab = rs.clusters(1)
    sizes = np.bincount(lab, minlength=rs.n)
    assert (sizes > 0).sum() == 18_857 and sizes.max() == 65_106 and (sizes == 1).sum() == 14_632
    assert (lab <= np.arange(rs.n)).all() and np.array_equal(lab[lab], lab)
    assert np.array_equal(rs.clusters(0), np.arange(rs.n))
    edges, vals, radius = rs.mst()
    assert radius == 2 and len(edges) == rs.n - 1 and (vals == 1).sum() == rs.n - 18_857
    assert (np.diff(vals) >= 0).all() and np.array_equal(vals, rs.values("n", edges[:, 0], edges[:, 1]))
    for v in (1, 2):   # ascending (distance, i, j)
        at = canon(rs.n, edges[vals == v, 0], edges[vals == v, 1])
        assert (np.diff(at) > 0).all()
    assert (canon(rs.n, edges[:, 0], edges[:, 1]) >= TWO32).sum() > 0   # forest edges past the 2^32 offset
    assert (edges[:, 0] >= 65_536).sum() > 0


@pytest.mark.parametrize("which", ["set", "tall"])
def test_windowed_closed_forms_are_the_oracles_tallies(rs, which):
    """every window of test_gpu_record_boundary_windows.py: the closed forms are the oracle's on the cut columns"""
    rs = rs if which == "set" else rbc.tall_set()
    rng = np.random.default_rng(8)
    rows = np.concatenate([rs.picked[:6], rs.picked[-6:], [rs.n - 3, rs.n - 2, rs.n - 1]])
    cols = np.concatenate([rng.choice(rs.n, 24, replace=False), rows[:3], [65_536, rs.n - 1, rs.n - 2]])   # (all residues, i == j)
    i, j = [x.ravel() for x in np.meshgrid(rows, cols, indexing="ij")]
    assert 300 <= len(i) <= 600 and (i == j).any()
    some = np.concatenate([rs.picked, rng.choice(rs.n, 200, replace=False)])
    for b, e in rbc.WINDOWS:
        for m in MEASURES:
            mine = rs.window_tallies(m, i, j, b, e)
            if e <= b:
                assert not mine.any(), (m, b, e)
                continue
            got = oracle.tallies_rect(m, rs.codes[rows, b:e], rs.codes[cols, b:e]).reshape(len(i), -1)
            assert np.array_equal(got, mine.astype(np.uint64)), (m, b, e)
        mine = rs.window_base_counts(b, e)
        direct = np.stack([(rs.codes[:, b:e] == code).sum(axis=1) for code in (rbc.A, 24, rbc.G, rbc.C)], axis=1)
        assert np.array_equal(mine, direct.astype(np.uint32)), (b, e)
        if e > b:
            assert np.array_equal(oracle.count_bases_matrix(rs.codes[some, b:e]), mine[some].astype(np.uint64)), (b, e)
            want = oracle.all_pairs_rect("raw", rs.codes[rows, b:e], rs.codes[cols, b:e]).ravel()
            got = rs.window_values("raw", i, j, b, e)
            assert np.array_equal(np.isnan(got), np.isnan(want)), (b, e)
            ok = ~np.isnan(want)
            assert np.array_equal(got[ok].view(np.uint64), want[ok].view(np.uint64)), (b, e)
        else:
            assert np.isnan(rs.window_values("raw", i, j, b, e)).all() and not rs.window_values("n", i, j, b, e).any()
    # the whole width is the unwindowed form, and the last two sites leave some pairs without a comparable site
    for m in MEASURES:
        assert np.array_equal(rs.window_tallies(m, i, j, 0, 40), rs.tallies(m, i, j)), m
    assert np.array_equal(rs.window_base_counts(0, 40), rs.base_counts())
    assert set(np.unique(rs.window_comparable(i, j, 38, 40))) == {0, 1, 2}
    assert set(rbc.NEAREST_WINDOWS) <= set(rbc.WINDOWS)


def test_window_cases_reach_what_they_claim(rs):
    """the constants of test_gpu_record_boundary_windows.py: a later change of one cannot silently empty a test"""
    n, tall = rs.n, rbc.TALL_RECORDS
    # d. more than 65,535 row tiles in one window launch, the second grid inside the set and, with the row begin, off a
    # multiple of 8; the slab cut of nearest_windows and of the stream keeps all the rows in one slab
    assert rbc.WIN_ROWS == 8 and tall == 524_289 and -(-tall // rbc.WIN_ROWS) > rbc.GRID_ROWS
    assert rbc.second_grid_first_row(0, tall) == 524_280 < tall
    assert rbc.second_grid_first_row(rbc.TALL_ROW_BEGIN, tall) == 524_283 < tall and 524_283 % 8 != 0
    assert rbc.second_grid_first_row(0, n) is None
    cols = rbc.tall_columns()
    assert len(cols) == 5 and cols[0] == 0 and cols[-1] == tall - 1 and (np.diff(cols) > 0).all()
    for n_windows in (1, 2):
        assert rbc.cut_window_slabs(tall, n_windows, len(cols)) == (tall, n_windows)   # nearest_windows, the stream
    ts = rbc.tall_set()
    assert ts.n == tall and len(np.unique(ts.words)) == tall and ts.codes.nbytes < 22 << 20
    # e. the cuts of nearest_windows on 10 rows x 3 windows x 92,700 columns: one list; a few rows of all windows; all rows
    assert rbc.cut_window_slabs(10, 3, n, 1) == (1, 1)
    assert rbc.cut_window_slabs(10, 3, n, n * 16) == (5, 3)
    assert rbc.cut_window_slabs(10, 3, n) == (10, 3)
    # f. the stream's ranges of the loaded 92,700 x 3 windows at batches of 128: two ranges of rows, each one grid
    rows, wins = rbc.cut_window_slabs(n, 3, 128)
    assert wins == 3 and n / 2 < rows < n and rbc.second_grid_first_row(0, rows) is None
    # c. the square list: positions at or above 2^32, both sides of row 65,536, the diagonal, both orders, repeats
    row, col = rbc.boundary_pairs()
    lo, hi = np.minimum(row, col), np.maximum(row, col)
    off = lo != hi
    at = canon(n, lo[off], hi[off])
    assert at.max() == n * (n - 1) // 2 - 1 == 4_296_598_649 and (at >= TWO32).sum() > 100 and (at < TWO32).sum() > 100
    assert (lo == 65_535).any() and (lo == 65_536).any() and (~off).sum() == 4
    assert (row < col).sum() > 1_000 and (row > col).sum() > 1_000 and not (np.diff(at) >= 0).all()
    assert len(np.unique(at)) < off.sum() // 2 + 1   # every pair at least twice
    assert lo[off].min() >= 65_530 and ((lo >= 65_545) & (lo < 90_890)).sum() == 0 and hi.max() == n - 1
    default = rbc.touched_slabs(n, 1 << 25, row, col)
    at_row = rbc.touched_slabs(n, rbc.max_pairs_cutting_in(n, 65_536, 65_536), row, col)
    past = rbc.touched_slabs(n, rbc.max_pairs_cutting_in(n, FIRST_ROW_PAST_2_32, n - 2), row, col)
    assert 2 <= len(default) <= 6 and 2 <= len(at_row) <= 6 and 2 <= len(past) <= 6
    assert any(s[1] == 65_536 for s in at_row) and any(s[0] == 65_536 for s in at_row)
    assert past[-1][2] >= TWO32 and default[-1][2] < TWO32 < default[-1][2] + default[-1][3]
    # c. the rectangle list: positions i n + j either side of 2^32
    row, col = rbc.boundary_rect_pairs()
    at = row * n + col
    assert rbc.FIRST_RECT_ROW_PAST_2_32 * n >= TWO32 > (rbc.FIRST_RECT_ROW_PAST_2_32 - 1) * n
    assert (at == TWO32 - 1).sum() == 1 and (at == TWO32).sum() == 1 and (at >= TWO32).sum() == len(at) - 1
    assert (row == col).sum() == 2 and at.max() == n * n - 1 and (row >= 65_536).any() and (col >= 65_536).any()
    assert len(np.unique(row // 300)) <= 6   # (a slab of the default bound holds 361 rows)


def greedy_cut(n, max_pairs):
    """cut_row_slabs of the engine (square), loop by loop in Python integers"""
    slabs, first, rb = [], 0, 0
    while rb < n:
        re, pairs = rb, 0
        while re < n:
            row_pairs = n - re - 1
            if re > rb and pairs + row_pairs > max_pairs:
                break
            pairs += row_pairs
            re += 1
        if pairs:
            slabs.append((rb, re, first, pairs))
        first += pairs
        rb = re
    return slabs


def test_slab_cuts_the_gpu_tests_ask_for(rs):
    n = rs.n
    two = greedy_cut(n, rbc.TWO_SLAB_MAX_PAIRS)
    assert two == rbc.cut_row_slabs(n, rbc.TWO_SLAB_MAX_PAIRS)
    assert len(two) == 2 and two[1][1] - two[1][0] == 65_539 > rbc.GRID_ROWS and two[0][1] == 27_161
    assert two[1][3] == 2_147_647_491 and two[1][3] * 8 < 18 << 30   # the second grid's rows, a 17.2 GB slab of payloads
    small = rbc.max_pairs_cutting_in(n, 65_536, 65_536)
    cut = greedy_cut(n, small)
    assert small == 38_540_932 and cut == rbc.cut_row_slabs(n, small) and len(cut) == 112
    assert any(s[1] == 65_536 for s in cut) and any(s[0] == 65_536 and s[2] == 3_927_670_784 for s in cut)
    # the analyses' default bound: the last slab begins below 2^32 and ends above it
    default = greedy_cut(n, 1 << 25)
    assert len(default) == 129 and default[-1][2] < TWO32 < default[-1][2] + default[-1][3]
    assert sum(s[3] for s in default) == n * (n - 1) // 2
    # a bound whose last slab begins at or above 2^32: its out_base needs 33 bits
    past = rbc.max_pairs_cutting_in(n, FIRST_ROW_PAST_2_32, n - 2)
    cut = greedy_cut(n, past)
    assert cut == rbc.cut_row_slabs(n, past) and cut[-1][0] >= FIRST_ROW_PAST_2_32 and cut[-1][2] >= TWO32
    assert (past, len(cut), cut[-1][0]) == PAST_2_32_CUT
