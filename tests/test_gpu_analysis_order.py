"""GPU (-m gpu): the slab-driven analyses share one slab scratch per context (dst_ctx::pair_slab) — a 16 B/pair tally
slab (nearest, the finish of mst) and an 8 B/pair payload slab (clusters, mst's rounds, nj, dendrogram) follow each other
through it in both orders, across uploads of a larger and a smaller set.  Every result must be bit-identical to the same
call on a fresh context: the library against itself, because the order of calls is what is under test (the suites of
the single analyses hold them against their references)."""
import numpy as np
import pytest

import distance_amd as da
from helpers import random_alignment

pytestmark = pytest.mark.gpu

# max_pairs=500: dozens of slabs with a short last one (nearest has no such knob: one slab)
OPS = (
    ("nearest", lambda e: e.nearest("tn93", k=3, tallies=True)),
    ("clusters", lambda e: e.clusters("n_high", 3.0, max_pairs=500)),
    ("mst tallies", lambda e: e.mst("tn93", max_pairs=500, tallies=True)),
    ("mst", lambda e: e.mst("raw", max_pairs=500)),
    ("nj", lambda e: e.nj("k80", max_pairs=500)),
    ("dendrogram", lambda e: e.dendrogram("raw", "average", max_pairs=500)),
)


def same(a, b):
    if isinstance(a, np.ndarray):
        if a.dtype != b.dtype or a.shape != b.shape:
            return False
        if a.dtype == np.float64:   # bit for bit, NaN included
            return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))
        return np.array_equal(a, b)
    return a == b


@pytest.fixture(scope="module")
def sets():
    return {"large": random_alignment(193, 300, seed=71), "small": random_alignment(97, 300, seed=72)}


@pytest.fixture(scope="module")
def fresh(sets):
    """(set, operation) -> the result on a context that has run nothing else."""
    out = {}
    for tag, codes in sets.items():
        for name, op in OPS:
            with da.Engine() as eng:
                eng.upload(0, codes)
                out[tag, name] = op(eng)
    return out


def run_and_compare(eng, tag, ops, fresh, step):
    for name, op in ops:
        got, want = op(eng), fresh[tag, name]
        assert len(got) == len(want), (step, tag, name)
        for k, (g, w) in enumerate(zip(got, want)):
            assert same(g, w), (step, tag, name, k)


def test_six_analyses_forwards_then_backwards_on_one_context(sets, fresh):
    with da.Engine() as eng:
        eng.upload(0, sets["large"])
        run_and_compare(eng, "large", OPS, fresh, "forwards")
        run_and_compare(eng, "large", OPS[::-1], fresh, "backwards")


def test_analyses_across_uploads_of_a_smaller_and_a_larger_set(sets, fresh):
    with da.Engine() as eng:
        eng.upload(0, sets["large"])
        run_and_compare(eng, "large", OPS[:1], fresh, "large, nearest only")
        eng.upload(0, sets["small"])
        run_and_compare(eng, "small", OPS, fresh, "small, forwards")
        eng.upload(0, sets["large"])
        run_and_compare(eng, "large", OPS[::-1], fresh, "large again, backwards")
