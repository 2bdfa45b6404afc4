"""Host only: oracle.tallies_rect (orc_tallies_rect, the threaded loop the sequence tests read whole rows of tallies from)
gives what oracle.tallies gives pair by pair — every measure, any thread count, rows any stride apart."""
import numpy as np
import pytest

import oracle
from helpers import random_alignment, uniform_codes

ALL = ("n", "n_high", "raw", "jc69", "k80", "tn93")


@pytest.mark.parametrize("threads", [1, 3, 64, 1000])
def test_every_pair_as_the_per_pair_call(threads):
    a, b = random_alignment(7, 301, 1), uniform_codes(11, 301, 2)
    for m in ALL:
        got = oracle.tallies_rect(m, a, b, threads=threads)
        assert got.shape == (7, 11, oracle.N_TALLIES[m]) and got.dtype == np.uint64
        for i in range(7):
            for j in range(11):
                assert list(got[i, j]) == [int(x) for x in oracle.tallies(m, a[i], b[j])], (m, i, j)


def test_rows_any_stride_apart_and_single_rows():
    wide_a, wide_b = uniform_codes(9, 400, 3), random_alignment(6, 500, 4)
    a, b = wide_a[::2, 50:250], wide_b[1:, 300:500]          # views: row strides of 800 and 500 bytes, 200 sites
    assert not a.flags.c_contiguous and not b.flags.c_contiguous
    for view_a, view_b in ((a, b), (np.ascontiguousarray(a)[2:3], b), (a, np.ascontiguousarray(b)[:1])):
        got = oracle.tallies_rect("tn93", view_a, view_b, threads=4)
        for i in range(len(view_a)):
            for j in range(len(view_b)):
                assert list(got[i, j]) == [int(x) for x in oracle.tallies("tn93", view_a[i], view_b[j])], (i, j)
    assert oracle.tallies_rect("k80", a[:0], b, threads=4).shape == (0, 5, 3)
