"""CPU: the host side of dst_links: the declaration and the export, the ABI version, the chunk constant in the header and
in Python, the NULL-context status, and the numpy restatement of the link rule against a hand-written example."""
import re

import numpy as np

import distance_amd as da
from distance_amd import _lib
from links_reference import components, expected, linked

ERR_ARG = 1


def test_declared_and_exported():
    assert "dst_links" in da.declared_symbols()
    lib = da.load()
    assert hasattr(lib, "dst_links")
    assert "dst_links" in _lib._SIGS


def test_abi_version_stays_3():
    assert da.load().dst_abi_version() == 3


def test_chunk_constant_matches_header():
    text = open(_lib.HEADER_PATH).read()
    m = re.search(r"#define\s+DST_LINKS_CHUNK\s+\(1u\s*<<\s*(\d+)\)", text)
    assert m and (1 << int(m.group(1))) == da.LINKS_CHUNK == _lib.LINKS_CHUNK == 4194304
    assert re.search(r"#define\s+DST_LINKS_VALUES\s+1\b", text) and _lib.LINKS_VALUES == 1
    assert re.search(r"#define\s+DST_LINKS_TALLIES\s+2\b", text) and _lib.LINKS_TALLIES == 2


def test_null_context_is_err_arg():
    lib = da.load()
    assert lib.dst_links(None, 2, 1, 0, 1, 1.0, 0, 0, None, None, None) == ERR_ARG


def test_reference_on_a_hand_written_example():
    # 5 records, canonical order (0,1) (0,2) (0,3) (0,4) (1,2) (1,3) (1,4) (2,3) (2,4) (3,4)
    v = np.array([3, 0, 7, 2, 5, 2, 9, 6, 2, 4], np.int64)
    r, c, w = expected("n", v, 5, 5, True, 2.9)   # floor(2.9) = 2
    assert list(zip(r, c)) == [(0, 2), (0, 4), (1, 3), (2, 4)] and list(w) == [0, 2, 2, 2]
    assert r.dtype == np.uint32 and c.dtype == np.uint32
    assert list(components(5, r, c)) == [0, 1, 0, 1, 0]
    assert not linked("n_high", v, -1e300).any() and linked("n_high", v, 1e300).all()
    f = np.array([0.5, -0.0, np.nan, np.inf, 0.0, 0.25], np.float64)   # a 2 x 3 rectangle
    r, c, w = expected("raw", f.reshape(2, 3), 2, 3, False, 0.0)
    assert list(zip(r, c)) == [(0, 1), (1, 1)] and np.signbit(w[0]) and not np.signbit(w[1])
    r, c, w = expected("jc69", f, 2, 3, False, np.inf)
    assert list(zip(r, c)) == [(0, 0), (0, 1), (1, 0), (1, 1), (1, 2)]
    r, c, w = expected("raw", f, 2, 3, False, 0.3)
    assert list(zip(r, c)) == [(0, 1), (1, 1), (1, 2)]
