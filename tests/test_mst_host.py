"""CPU: dst_mst's surface without a GPU — the symbol is declared and exported, the ABI version stays — and the host
reference (tests/mst_reference.py) against hand-made matrices and its own cut property."""
import numpy as np
import pytest

import distance_amd as da
from mst_reference import components, condensed, kruskal, linked, nn_key

INF, NAN = float("inf"), float("nan")


def test_symbol_declared_and_exported():
    assert "dst_mst" in da.declared_symbols()
    assert hasattr(da.load(), "dst_mst")


def test_abi_version_unchanged():
    assert da.load().dst_abi_version() == 3


def test_nn_key_order():
    v = np.array([-INF, -2.0, -1e-300, -0.0, 0.0, 1e-300, 1.0, INF, NAN])
    k = nn_key(v)
    assert k[3] == k[4]
    assert all(int(k[a]) < int(k[a + 1]) for a in (0, 1, 2, 4, 5, 6, 7))
    assert int(k[8]) == 2 ** 64 - 1
    assert int(nn_key(np.array([np.copysign(NAN, -1.0)]))[0]) == 2 ** 64 - 1   # a NaN of either sign
    ki = nn_key(np.array([-5, 0, 7], np.int64))
    assert int(ki[0]) < int(ki[1]) < int(ki[2])


def test_all_equal_gives_the_star_at_zero():
    for n, dtype in ((7, np.float64), (12, np.int64)):
        vals = np.full(n * (n - 1) // 2, 3, dtype)
        edges, values = kruskal(n, vals)
        assert edges.tolist() == [[0, j] for j in range(1, n)]
        assert values.dtype == dtype and (values == 3).all()


def test_one_nan_row_gives_a_forest():
    n, dead = 9, 4
    rng = np.random.default_rng(1)
    m = rng.random((n, n))
    m[dead, :] = NAN
    m[:, dead] = NAN
    edges, values = kruskal(n, condensed(m))
    assert len(edges) == n - 2
    assert dead not in edges
    assert not np.isnan(values).any()
    assert len(np.unique(components(n, edges[:, 0], edges[:, 1]))) == 2


def test_signed_zeros_tie_and_fall_to_ij():
    # a triangle of zeros of both signs and one larger value: the order of the zero edges rests on (i, j) alone
    m = np.zeros((4, 4))
    m[0, 1], m[0, 2], m[1, 2] = 0.0, -0.0, -0.0
    m[0, 3], m[1, 3], m[2, 3] = 5.0, -0.0, 0.0
    edges, values = kruskal(4, condensed(m))
    assert edges.tolist() == [[0, 1], [0, 2], [1, 3]]
    assert np.signbit(values).tolist() == [False, True, True]   # the values keep their own sign


def test_inf_is_an_edge():
    m = np.full((3, 3), NAN)
    m[0, 1], m[0, 2], m[1, 2] = INF, NAN, 1.0
    edges, values = kruskal(3, condensed(m))
    assert edges.tolist() == [[1, 2], [0, 1]]
    assert values.tolist() == [1.0, INF]


def test_tiny():
    e, v = kruskal(1, np.zeros(0))
    assert e.shape == (0, 2) and len(v) == 0
    e, v = kruskal(2, np.array([NAN]))
    assert e.shape == (0, 2)
    e, v = kruskal(2, np.array([2], np.int64))
    assert e.tolist() == [[0, 1]] and v.tolist() == [2]


@pytest.mark.parametrize("seed", [2, 3, 4])
def test_cut_property(seed):
    """For every T the components of the forest's edges with v <= T are the components of all pairs with v <= T."""
    rng = np.random.default_rng(seed)
    n = 40
    vals = rng.integers(0, 12, n * (n - 1) // 2).astype(np.float64)   # many ties
    vals[rng.random(len(vals)) < 0.2] = NAN
    vals[rng.random(len(vals)) < 0.05] = INF
    vals[(vals == 0) & (rng.random(len(vals)) < 0.5)] = -0.0
    edges, values = kruskal(n, vals)
    keys = [int(k) for k in nn_key(values)]
    assert keys == sorted(keys)
    i, j = np.triu_indices(n, 1)
    for t in (-1.0, 0.0, 3.0, 7.5, 11.0, 1e9, INF):
        full = linked(vals, t)
        cut = linked(values, t)
        assert np.array_equal(components(n, edges[cut, 0], edges[cut, 1]), components(n, i[full], j[full])), t
    ints = rng.integers(0, 6, n * (n - 1) // 2).astype(np.int64)
    edges, values = kruskal(n, ints)
    assert len(edges) == n - 1
    for t in (-1.0, 0.0, 2.5, 5.0):
        full, cut = linked(ints, t), linked(values, t)
        assert np.array_equal(components(n, edges[cut, 0], edges[cut, 1]), components(n, i[full], j[full])), t
