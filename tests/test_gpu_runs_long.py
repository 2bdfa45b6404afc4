"""GPU (-m gpu): run records (dst_internal.h: RunIndex) on long alignments.

The run records' correction tables come from two kernels: chunk_sums_kernel (every record's per-chunk sums, one LDS row
per wave and accumulator word) and corr_mfma_kernel (those sums times the run masks, in rounds of 8 mask words).  With one
LDS row over ALL chunks, 4 waves x W words x kpad chunks x 4 bytes, the first kernel needed more than 64 KiB from 131,073
sites on (tn93, W = 4) and more than a CU's 160 KiB from 327,681 (k80: 434,177; raw / jc69: 655,361; n / n_high:
1,310,721), where its launch is refused.  It now walks the chunks in slices of kSumSliceChunks = 1,024 (SLICE below).

Few records (24, of which 7 are run records: max_run is n / 3), masks written by hand so that every edge is met at every
length: run chunks 0..3 only; a run to the alignment's end (L is not always a multiple of 128: the last chunk is partial,
its padding counts as N); exactly four run chunks across chunk 2,559 | 2,560 (the last the first form could serve at W = 4);
four across every slice boundary; two run records whose runs overlap above chunk 2,560 (the F term) and two whose runs are
disjoint; a record with three whole chunks of N between unaligned ends (below kRunMin: it stays plain); a record half N
(hundreds of mask words); a column of ambiguity codes and scattered gaps across the runs.  Every measure, distances and
tallies, bit for bit against the dense kernels; those sampled against the oracle; and the run records are KEPT."""
import functools

import numpy as np
import pytest

import distance_amd as da
import oracle
from helpers import random_alignment

pytestmark = pytest.mark.gpu
ALL = ("n", "n_high", "raw", "jc69", "k80", "tn93")
TALLIED = ("raw", "k80", "tn93")
N = 24
SLICE = 1024          # kSumSliceChunks (dst_internal.h): chunks of one slice of chunk_sums_kernel
OLD_LAST = 2560       # 160 KiB / (4 waves x 4 words x 4 bytes): chunks the one-row form could hold at W = 4
# the records with designed masks
R_HEAD, R_TAIL, R_OLD, R_SLICE, R_OVER_A, R_OVER_B, R_HALF, P_THREE, P_GAPS = 1, 2, 3, 4, 5, 6, 7, 8, 10
RUN_RECORDS = (R_HEAD, R_TAIL, R_OLD, R_SLICE, R_OVER_A, R_OVER_B, R_HALF)
# lengths: mask_words of 8 (one whole round of corr_mfma_kernel, narrow tallies), 9 (one word past it), 16 (two rounds, the
# first wide length), 18 with a last chunk of one site; the 64 KiB boundary of tn93 (131,072 | 131,073: also the first slice
# boundary) and of k80; the 160 KiB boundary of tn93 (327,680 | 327,681), k80, raw / jc69 and n / n_high
LENGTHS = (32_768, 32_769, 65_536, 69_633, 131_072, 131_073, 172_033, 327_680, 434_177, 655_361, 1_310_721, 327_681)   # (the last one's
# reference serves the text test too)


def run_chunks(nch):
    """record -> [first run chunk, one past the last) of every designed run"""
    old = OLD_LAST if nch > OLD_LAST + 2 else nch // 2
    bounds = list(range(SLICE, nch, SLICE))                 # (a boundary before the last, partial chunk: the four end there)
    over = OLD_LAST + 40 if nch > OLD_LAST + 140 else nch // 2 + 8
    return {R_HEAD: [(0, 4)],
            R_TAIL: [(nch - 5, nch)],
            R_OLD: [(old - 2, old + 2)],
            R_SLICE: [(min(b + 2, nch) - 4, min(b + 2, nch)) for b in bounds] or [(nch // 3, nch // 3 + 4)],
            R_OVER_A: [(over, over + 40)],
            R_OVER_B: [(over + 24, over + 70)],
            R_HALF: [(nch // 4, nch // 4 + nch // 2)]}


def designed(L, hot=False):
    codes = random_alignment(N, L, 1000 + L % 997, p_ambig=0.002, p_gap=0.004, divergence=0.015)
    nch = (L + 127) // 128
    plan = run_chunks(nch)
    a0 = 128 * plan[R_OVER_A][0][0]
    codes[:, a0 + 128 * 30 + 5] = 192                                       # a column of R where both overlapping runs pass
    codes[P_GAPS, a0:a0 + 128 * 70:97] = 244                                # scattered gaps across them
    fill = {R_OLD: 242, R_SLICE: 244}                                       # (N, - and ? are one class)
    for r, spans in plan.items():
        for b, e in spans:
            codes[r, 128 * b:min(128 * e, L)] = fill.get(r, 240)
    codes[P_THREE, 128 * 20 - 37:128 * 23 + 51] = 240                       # three whole chunks and two partial ones
    if hot:   # clade-like columns: a third of the records share G at every 40th site (the hybrid path's hot sites)
        codes[:N // 3, ::40] = np.where(codes[:N // 3, ::40] >= 240, codes[:N // 3, ::40], 72)
    codes.setflags(write=False)
    return codes


def host_run_records(codes):
    """records with kRunMin = 4 or more whole 128-site chunks of N; sites past the alignment's end count as N"""
    n, L = codes.shape
    nch = (L + 127) // 128
    padded = np.full((n, nch * 128), 240, np.uint8)
    padded[:, :L] = codes
    whole = ((padded >> 4) == 15).reshape(n, nch, 128).all(axis=2).sum(axis=1)
    return [int(r) for r in np.flatnonzero(whole >= 4)]


@functools.lru_cache(maxsize=1)
def case(L, hot=False):
    """the alignment and the dense kernels' whole triangle of it (computed once, shared, read-only)"""
    codes = designed(L, hot)
    with da.Engine(0) as ref:
        ref.set_path("dense")
        ref.upload(0, codes)
        want = {m: ref.run_square(m) for m in ALL}
        want_t = {m: ref.run_square(m, tallies=True) for m in TALLIED}
        assert ref.last_path() == "dense"
    for a in list(want.values()) + list(want_t.values()):
        a.setflags(write=False)
    return codes, want, want_t


def pair_at(i, j):
    return da.square_row_start(N, i) + j - i - 1


@pytest.fixture(scope="module")
def eng():
    e = da.Engine(0)
    yield e
    e.close()


def check_against_dense(eng, codes, want, want_t, path):
    """upload as the default does (fused preparation: the pack strips the run records), then every measure on `path`"""
    expect = host_run_records(codes)
    assert expect == list(RUN_RECORDS)                      # (the design: P_THREE stays plain)
    eng.set_prep_threshold(0)
    try:
        eng.set_path("auto")
        eng.upload(0, codes)
        eng.set_path(path)
        for m in ALL:
            got = eng.run_square(m)
            assert eng.last_path() == path, (m, eng.last_path())
            assert eng.last_launch()["run_records"] == 1, m
            assert np.array_equal(got, want[m], equal_nan=True), (m, int((got != want[m]).sum()))
            assert eng.run_records()[0] == len(expect), (m, eng.run_records())
        for m in TALLIED:
            got = eng.run_square(m, tallies=True)
            assert np.array_equal(got, want_t[m]), (m, np.flatnonzero((got != want_t[m]).reshape(len(got), -1).any(axis=1))[:8])
        n_run, removed = eng.run_records()
        assert n_run == len(expect) and removed > 0, (n_run, removed)
    finally:
        eng.set_prep_threshold(2e10)
        eng.set_path("auto")


# run x run (disjoint, overlapping, inside the half-N record), run x plain, plain x run, and the record below kRunMin
ORACLE_PAIRS = ((R_HEAD, R_TAIL), (R_OVER_A, R_OVER_B), (R_OLD, R_HALF), (R_SLICE, R_HALF), (R_OVER_B, R_HALF),
                (R_TAIL, P_GAPS), (R_HALF, P_THREE), (R_HALF, N - 1), (0, R_SLICE), (0, R_HALF), (P_THREE, P_GAPS), (R_OVER_A, P_GAPS))


@pytest.mark.parametrize("L", LENGTHS)
def test_run_records_on_long_alignments_give_the_dense_bits(eng, L):
    codes, want, want_t = case(L)
    for m in ("tn93", "raw"):                               # the dense reference itself against the oracle
        for i, j in ORACLE_PAIRS:
            assert list(want_t[m][pair_at(i, j)]) == [int(x) for x in oracle.tallies(m, codes[i], codes[j])], (m, i, j)
    check_against_dense(eng, codes, want, want_t, "consensus")


def test_text_of_a_run_records_row_past_the_old_limit(eng):
    """327,681 sites: the TSV text of the half-N record's row, from the device, equals the host's text of the dense tallies"""
    L, r = 327_681, R_HALF
    codes, _, want_t = case(L)
    ids = ["r%d" % k for k in range(N)]
    eng.set_prep_threshold(0)
    try:
        eng.set_path("auto")
        eng.upload(0, codes)
        eng.set_path("consensus")
        eng.set_ids(0, ids)
        text = eng.text_square("tn93", r, r + 1, capacity=1 << 20)
        assert eng.last_path() == "consensus" and eng.run_records()[0] == len(RUN_RECORDS)
    finally:
        eng.set_prep_threshold(2e10)
        eng.set_path("auto")
    tl = want_t["tn93"][pair_at(r, r + 1):pair_at(r, N - 1) + 1]
    host = oracle.finalize_square("tn93", tl, N, oracle.count_bases_matrix(codes), r, r + 1)
    assert text == oracle.tsv_square("tn93", host, ids, r, r + 1)


def test_hot_columns_and_run_records_past_the_old_limit(eng):
    """327,681 sites with clade-like columns on the hybrid path: the lists without the hot sites feed the same tables"""
    codes, want, want_t = case(327_681, True)
    for i, j in ORACLE_PAIRS[:6]:
        assert list(want_t["tn93"][pair_at(i, j)]) == [int(x) for x in oracle.tallies("tn93", codes[i], codes[j])], (i, j)
    check_against_dense(eng, codes, want, want_t, "hybrid")
