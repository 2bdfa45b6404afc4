"""GPU (-m gpu): NJ bootstrap support (dst_nj_bootstrap) against the restatement — replicate alignments built in numpy
from the restated column map, their trees from the NJ restatement (nj_reference.py), the support counted from leaf
bitmasks (bootstrap_reference.py) — and its invariances, its independence of the loaded slots, its error case and one
larger run."""
import numpy as np
import pytest

import bootstrap_reference as B
import distance_amd as da
import nj_reference as R
import oracle
from helpers import CODES, random_alignment
from tools import synth

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE, ERR_CAPACITY = 1, 4, 6
UMAX = 0xFFFFFFFF


@pytest.fixture(scope="module")
def eng():
    with da.Engine(0) as e:
        yield e


def alignment(n, L, seed, divergence=0.05):
    """N, gaps and ambiguity codes (random_alignment's noise), duplicate records, and one record that is mostly N"""
    codes = random_alignment(n, L, seed=seed, divergence=divergence, p_ambig=0.03, p_gap=0.03)
    rng = np.random.default_rng(seed)
    if n >= 5:
        src, dst = rng.integers(0, n, n // 5 + 1), rng.integers(0, n, n // 5 + 1)
        codes[dst] = codes[src]
        codes[n - 1, : L // 2] = CODES[14]
    return np.ascontiguousarray(codes)


def replicate_tree(eng, measure, rep):
    """the replicate's tree by the restatement: payloads from the pair kernels (n / n_high: the oracle's exact values)"""
    n = rep.shape[0]
    if measure in da.INT_MEASURES:
        payloads = oracle.all_pairs_square(measure, rep)
    else:
        eng.upload(0, rep)
        payloads = eng.run_square(measure)
    return R.nj(R.square(n, payloads))[0]


def check_support(eng, measure, codes, reps, seed, **kw):
    n = codes.shape[0]
    eng.upload(0, codes)
    main = eng.nj(measure)[0]
    support, trees = eng.nj_bootstrap(measure, codes, main, reps, seed=seed, trees=True, **kw)
    assert trees.shape == (reps, 2 * n - 2)
    want_trees = [replicate_tree(eng, measure, B.replicate(codes, seed, r)) for r in range(reps)]
    for r in range(reps):
        assert np.array_equal(trees[r], want_trees[r]), r
    want = B.support(main, want_trees, n)
    assert np.array_equal(support, want)
    assert (support[:n] == UMAX).all() and support[2 * n - 3] == UMAX
    assert (support[n:2 * n - 3] <= reps).all()
    return support, trees


# ---- 1. exact support ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", ["n", "raw", "k80", "tn93"])
@pytest.mark.parametrize("n,L", [(3, 300), (4, 450), (5, 700), (64, 1500), (257, 900)])
def test_exact_support(eng, measure, n, L):
    codes = alignment(n, L, seed=n * 7 + L)
    support, _ = check_support(eng, measure, codes, 16, seed=n + 11)
    if n >= 64:
        assert (support[n:2 * n - 3] == 16).any() and (support[n:2 * n - 3] < 16).any()


@pytest.mark.parametrize("measure", ["jc69", "n_high"])
def test_exact_support_low_divergence(eng, measure):
    codes = random_alignment(64, 1200, seed=77, divergence=0.02, p_ambig=0.01, p_gap=0.01)
    check_support(eng, measure, codes, 16, seed=5)


# Rows of up to 49,152 bytes are staged in LDS (boot_resample_kernel<true>), longer ones are gathered from global memory
# (<false>); a thread writes four columns as one 32-bit store, the last one N-padded when L is not a multiple of 4.
@pytest.mark.parametrize("L,measure,path", [(49152, "n_high", "auto"), (49153, "raw", "auto"), (49167, "n", "auto"),
                                            (65537, "n_high", "auto"), (65537, "raw", "consensus")])
def test_exact_support_beyond_the_staged_row(eng, L, measure, path):
    """the last staged size, the first rows gathered from global memory, L = 1 and 3 (mod 4) there, and 65,537 sites on
    the consensus path (one 32-bit word per tally)"""
    codes = alignment(24, L, seed=L, divergence=0.02)
    try:
        if path != "auto":
            eng.set_prep_threshold(0)
            eng.set_path(path)
        check_support(eng, measure, codes, 4, seed=L + 3)
        if path != "auto":
            # the bootstrap's own pair launches go through the context's launcher: the report right after a call is its
            # last replicate's fill, on the forced path with one 32-bit word per tally
            eng.upload(0, codes)
            main = eng.nj(measure)[0]
            eng.run_square(measure, 0, 1)                 # (a 23-pair launch, so that the report below is not this one)
            eng.nj_bootstrap(measure, codes, main, 2, seed=L + 3)
            li = eng.last_launch()
            assert li["path"] == path and li["wide"] == (L >= 65536) and li["pairs"] == 24 * 23 // 2, li
    finally:
        eng.set_path("auto")
        eng.set_prep_threshold(2e10)


@pytest.mark.parametrize("n,L", [(9, 301), (9, 303), (7, 15), (6, 17), (5, 1)])
def test_exact_support_of_odd_and_tiny_widths(eng, n, L):
    """L = 1 and 3 (mod 4): the tail of a row's last 32-bit store; a single site (n_high is finite whatever is drawn)"""
    codes = alignment(n, L, seed=n * 100 + L, divergence=0.2)
    check_support(eng, "n_high", codes, 8, seed=L)


def test_row_stride_larger_than_the_width(eng):
    """rows stride bytes apart with stride > len, the padding filled with a byte that is no Paradis code: a read past len
    would be DST_ERR_INVALID_CODE or another tree"""
    n, L, reps, seed = 12, 303, 6, 21
    codes = alignment(n, L, seed=5, divergence=0.1)
    eng.upload(0, codes)
    main = eng.nj("n_high")[0]
    want_support, want_trees = check_support(eng, "n_high", codes, reps, seed=seed)
    stride = L + 37
    padded = np.full((n, stride), 7, np.uint8)
    padded[:, :L] = codes
    view = padded[:, :L]
    assert view.strides == (stride, 1) and 7 not in CODES
    support = np.zeros(2 * n - 2, np.uint32)
    trees = np.zeros((reps, 2 * n - 2), np.uint32)
    rc = da.load().dst_nj_bootstrap(eng._h, da.MEASURES["n_high"], view.ctypes.data, n, L, stride, reps, seed, 0,
                                    main.ctypes.data, support.ctypes.data, trees.ctypes.data, 2 * n - 2)
    assert rc == 0, eng._lib.dst_last_error(eng._h)
    assert np.array_equal(trees, want_trees) and np.array_equal(support, want_support)


# ---- 2. invariance -------------------------------------------------------------------------------------------------
def test_invariance(eng):
    codes = alignment(120, 800, seed=3)
    eng.upload(0, codes)
    main = eng.nj("tn93")[0]
    want = eng.nj_bootstrap("tn93", codes, main, 6, seed=9, trees=True)
    try:
        for max_pairs in (1, 97, 1 << 30):
            got = eng.nj_bootstrap("tn93", codes, main, 6, seed=9, max_pairs=max_pairs, trees=True)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), max_pairs
        eng.set_prep_threshold(0)
        for path in ("dense", "consensus", "hybrid"):
            eng.set_path(path)
            got = eng.nj_bootstrap("tn93", codes, main, 6, seed=9, trees=True)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), path
    finally:
        eng.set_path("auto")
        eng.set_prep_threshold(2e10)
    # the same seed again: the same result; the trees alone give the support
    again = eng.nj_bootstrap("tn93", codes, main, 6, seed=9)
    assert np.array_equal(again, want[0])
    assert np.array_equal(want[0], B.support(main, list(want[1]), 120))
    other = eng.nj_bootstrap("tn93", codes, main, 6, seed=10, trees=True)
    assert not np.array_equal(other[1], want[1])


def test_run_records(eng):
    """records with long runs of N (run records on the consensus path) give the dense path's trees"""
    n, L = 300, 3000
    codes = synth.alignment(synth.SEED ^ 51, n, L)
    synth.apply_nruns(codes, synth.nrun_plan(51, n, L, 0.2, 0.3))
    eng.upload(0, codes)
    main = eng.nj("raw")[0]
    try:
        eng.set_path("dense")
        want = eng.nj_bootstrap("raw", codes, main, 4, seed=2, trees=True)
        eng.set_path("consensus")
        eng.set_prep_threshold(0)
        got = eng.nj_bootstrap("raw", codes, main, 4, seed=2, trees=True)
    finally:
        eng.set_path("auto")
        eng.set_prep_threshold(2e10)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    eng.upload(0, B.replicate(codes, 2, 3))
    assert np.array_equal(eng.nj("raw")[0], want[1][3])


# ---- 3. the slots are not touched ------------------------------------------------------------------------------------
def test_slots_untouched(eng):
    a, b = alignment(90, 600, seed=31), alignment(40, 600, seed=32)
    eng.upload(0, a)
    eng.upload(1, b)
    before = (eng.run_square("tn93"), eng.run_rect("k80", 0, 1), eng.nj("raw"), eng.run_records(0))
    other = alignment(70, 500, seed=33)
    eng.upload(0, other)   # (the main tree of another alignment, then back)
    other_main = eng.nj("raw")[0]
    eng.upload(0, a)
    eng.nj_bootstrap("raw", other, other_main, 3, seed=4)
    after = (eng.run_square("tn93"), eng.run_rect("k80", 0, 1), eng.nj("raw"), eng.run_records(0))
    assert np.array_equal(before[0].view(np.uint64), after[0].view(np.uint64))
    assert np.array_equal(before[1].view(np.uint64), after[1].view(np.uint64))
    assert np.array_equal(before[2][0], after[2][0])
    assert np.array_equal(before[2][1].view(np.uint64), after[2][1].view(np.uint64))
    assert before[3] == after[3]
    assert eng.set_info(0) == (90, 600) and eng.set_info(1) == (40, 600)


# ---- 4. errors ----------------------------------------------------------------------------------------------------
def test_non_finite_replicate(eng):
    n, L = 20, 400
    codes = random_alignment(n, L, seed=41)
    codes[6] = CODES[14]
    codes[:, 123] = 136
    codes[6, 123] = 136        # one resolved site: a replicate that does not draw column 123 has NaN raw distances
    eng.upload(0, codes)
    main = eng.nj("raw")[0]
    first = next(r for r in range(64) if 123 not in set(B.columns(7, r, L).tolist()))
    with pytest.raises(da.DistanceError) as e:
        eng.nj_bootstrap("raw", codes, main, 64, seed=7)
    assert e.value.status == ERR_STATE
    assert f"replicate {first}:" in e.value.message and "records 0 and 6" in e.value.message
    # the context goes on working
    R.check_tree(*eng.nj("raw"), n)
    ok = random_alignment(n, L, seed=42)
    eng.upload(0, ok)
    check_support(eng, "raw", ok, 4, seed=7)


def test_arguments(eng):
    lib, h = da.load(), eng._h
    codes = random_alignment(6, 50, seed=1)
    eng.upload(0, codes)
    main = eng.nj("raw")[0]
    sup = np.zeros(10, np.uint32)

    def call(measure=2, c=codes, n=6, L=50, stride=50, reps=2, parent=main, support=sup, cap=10):
        return lib.dst_nj_bootstrap(h, measure, c.ctypes.data if c is not None else None, n, L, stride, reps, 1, 0,
                                    parent.ctypes.data if parent is not None else None,
                                    support.ctypes.data if support is not None else None, None, cap)

    assert call() == 0
    assert call(reps=0) == ERR_ARG and call(reps=10001) == ERR_ARG
    assert call(measure=9) == ERR_ARG and call(n=2) == ERR_ARG and call(stride=49) == ERR_ARG
    assert call(parent=None) == ERR_ARG and call(support=None) == ERR_ARG and call(c=None) == ERR_ARG
    assert call(cap=9) == ERR_CAPACITY
    bad = main.copy()
    bad[2] = 17                # out of range
    assert call(parent=bad) == ERR_ARG
    bad = main.copy()
    bad[0] = UMAX              # two roots
    assert call(parent=bad) == ERR_ARG
    wrong = codes.copy()
    wrong[3, 17] = 7           # not a Paradis code
    assert call(c=wrong) == 3   # DST_ERR_INVALID_CODE, as dst_upload
    assert call() == 0


# ---- 5. scale ------------------------------------------------------------------------------------------------------
def test_scale_2000(eng):
    n, L = 2000, 5000
    codes = synth.alignment(synth.SEED ^ 61, n, L)
    eng.upload(0, codes)
    main = eng.nj("raw")[0]
    support, trees = eng.nj_bootstrap("raw", codes, main, 4, seed=1, trees=True)
    for r in range(4):
        R.check_tree(trees[r], np.zeros(2 * n - 2), n)
    assert np.array_equal(support, B.support(main, list(trees), n))
    eng.upload(0, B.replicate(codes, 1, 2))
    assert np.array_equal(eng.nj("raw")[0], trees[2])
