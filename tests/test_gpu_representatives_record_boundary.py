"""GPU (-m gpu): dst_representatives on the designed set of record_boundary_cases.py: 92,700 records, 4,296,598,650 pairs,
`n_high` at T = 1.  Record indices need 17 bits and canonical ordinals 33; at the default slab bound the last slab straddles
offset 2^32, and at TWO_SLAB_MAX_PAIRS one slab has more than 65,535 rows (more than 128 sub-blocks behind one pair
kernel) and pair offsets above 2^32.  The reference is exact and needs no brute force: two records are within 1 exactly when their words
differ in one bit, so the sequential pass looks at each record's at most 20 one-bit-flip neighbours through the set's
word -> record table."""
import numpy as np
import pytest

import distance_amd as da
import record_boundary_cases as rbc
import representatives_reference as rr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rs():
    return rbc.record_set()


@pytest.fixture(scope="module")
def want(rs):
    flips = (np.uint32(1) << np.arange(rbc.BITS, dtype=np.uint32))

    def neighbours(i):
        nb = rs.table[rs.words[i] ^ flips]
        return nb[nb >= 0]

    rep = rr.greedy_from_neighbours(rs.n, neighbours)
    own = np.arange(rs.n)
    assert rep[0] == 0 and 1 < (rep == own).sum() < rs.n
    member = rep != own
    assert (rbc.POP[rs.xor(rep[member], own[member])] == 1).all()
    return rep.astype(np.uint32)


@pytest.fixture(scope="module")
def eng(rs):
    e = da.Engine(0)
    e.upload(0, rs.codes)
    yield e
    e.close()


def assert_result(rs, want, rep, values, tallies=None):
    own = np.arange(rs.n)
    member = want != own
    assert np.array_equal(rep, want)
    assert values.dtype == np.int64 and np.array_equal(values, member.astype(np.int64))   # all 1 for members, 0 bits else
    if tallies is not None:
        assert np.array_equal(tallies[:, 0], member.astype(np.uint32))


def test_default_slabs(eng, rs, want):
    rep, values, tallies = eng.representatives("n_high", 1, tallies=True)
    assert_result(rs, want, rep, values, tallies)
    assert eng.last_representatives == int((want == np.arange(rs.n)).sum())


def test_two_slabs_of_more_than_65535_rows(eng, rs, want):
    slabs = rbc.cut_row_slabs(rs.n, rbc.TWO_SLAB_MAX_PAIRS)
    assert len(slabs) == 2 and slabs[1][1] - slabs[1][0] > rbc.GRID_ROWS
    assert slabs[1][2] + slabs[1][3] > rbc.TWO32
    rep, values = eng.representatives("n_high", 1, max_pairs=rbc.TWO_SLAB_MAX_PAIRS)
    assert_result(rs, want, rep, values)
