"""CPU: the host side of dst_pair_sites: the declaration and the export, the signature, the ABI version, the NULL-context
status, the two constants, and the numpy predicate of pair_sites_reference against dst_site_tallies on every code pair."""
import ctypes as C
import re

import numpy as np
import pytest

import distance_amd as da
from distance_amd import _lib
from helpers import CODES
from pair_sites_reference import DIFF_WORDS, expected, listed, render

ERR_ARG = 1


def test_declared_and_exported():
    assert "dst_pair_sites" in da.declared_symbols()
    assert hasattr(da.load(), "dst_pair_sites")
    assert "dst_pair_sites" in _lib._SIGS and len(_lib._SIGS["dst_pair_sites"][1]) == 13


def test_abi_version_stays_3():
    assert da.load().dst_abi_version() == 3


def test_null_context_is_err_arg():
    one = (C.c_uint32 * 1)(0)
    off = (C.c_uint64 * 2)(0, 0)
    assert da.load().dst_pair_sites(None, 2, 1, 0, 1, C.addressof(one), C.addressof(one), 1, C.addressof(off), None, None, 0,
                                    None) == ERR_ARG


def test_constants_match_header():
    text = open(_lib.HEADER_PATH).read()
    m = re.search(r"#define\s+DST_PAIR_SITES_BATCH\s+\(1u\s*<<\s*(\d+)\)", text)
    assert m and (1 << int(m.group(1))) == da.PAIR_SITES_BATCH == _lib.PAIR_SITES_BATCH == 2 ** 20
    m = re.search(r"#define\s+DST_PAIR_SITES_WINDOW\s+\(1u\s*<<\s*(\d+)\)", text)
    assert m and (1 << int(m.group(1))) == da.PAIR_SITES_WINDOW == _lib.PAIR_SITES_WINDOW == 2 ** 24


@pytest.mark.parametrize("measure", da.MEASURES)
def test_predicate_is_the_difference_tally_of_dst_site_tallies(measure):
    lib = da.load()
    m = lib.dst_measure_from_name(measure.encode())
    width = lib.dst_tally_width(m)
    out = (C.c_int * 4)()
    q, t = np.meshgrid(CODES, CODES, indexing="ij")
    got = listed(measure, q >> 4, t >> 4)
    assert got.shape == (17, 17)
    for x in range(17):
        for y in range(17):
            assert lib.dst_site_tallies(m, int(CODES[x]), int(CODES[y]), out) == 0
            tally = sum(out[w] for w in DIFF_WORDS[measure])
            assert max(DIFF_WORDS[measure]) < width and tally in (0, 1)
            assert bool(got[x, y]) == (tally == 1), (measure, int(CODES[x]), int(CODES[y]))


def test_reference_on_a_hand_written_example():
    # A C G T R N      against      A T A Y Y A
    a = np.array([[136, 40, 72, 24, 192, 240]], np.uint8)
    b = np.array([[136, 24, 136, 48, 48, 136]], np.uint8)
    off, sites, bases = expected("n", a, b, [0], [0])
    assert list(off) == [0, 3] and list(sites) == [1, 2, 4] and list(bases) == [0x21, 0x48, 0xC3]
    assert render(sites, bases, 0, 3) == "C2T,G3A,R5Y" and render(sites, bases, 3, 3) == "."
    off, sites, bases = expected("k80", a, b, [0, 0], [0, 0])
    assert list(off) == [0, 3, 6] and list(sites) == [1, 2, 4] * 2
    off, sites, bases = expected("tn93", a, b, [0], [0])
    assert list(off) == [0, 2] and list(sites) == [1, 2]
    off, sites, bases = expected("raw", a, a, [], [])
    assert list(off) == [0] and sites.size == 0 and bases.size == 0
