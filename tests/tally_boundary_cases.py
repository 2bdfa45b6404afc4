"""Designed alignments on either side of the 16-bit tally switch (65,535 / 65,536 sites): plain numpy, no GPU.

Every pair kernel has a narrow form (len <= 65,535: two tallies in one 32-bit word, 16-bit hot tallies, DST_OUT_TALLY16,
the uint16 text kernels) and a wide form (len >= 65,536: one tally per word).  `boundary_alignment(L, kind)` builds a set
whose pairs drive every tally slot of every family to 0, 32,768, L - 32,768 and L itself, so that at L = 65,535 the
packed halves are all ones, a low half overflows into the high half before the corrections bring it back, and the high
half borrows.  test_tally_boundary_host.py asserts on the oracle alone that the set holds those patterns;
test_gpu_tally_boundary.py runs it through every path and reader.

Why 224 records and not fewer.  The engine's own rules decide what a set must look like to reach the code under test:
  * a site is hot when more than 5 % of the records deviate from the per-site plurality (kHotPermille), and the hybrid
    path runs only while at most half of the sites are hot.  The twelve extreme records deviate at ten records per site
    (see `deviants` below), the majority's mutations are laid out one record per site at most, so a cold site has 10 or
    11 deviants: below 5 % of 224 (11.2).  A hot column has the six clade records on top: 16 or 17.
  * the fused preparation (dst_set_prep_threshold(0)) counts lists, and makes run records, only while the records
    deviate at no more than 8 % of the sites on average (kListsMaxDeviation): 17.9 deviants per site of 224; "runs" has
    15 or 16, "hot" 13 on average.
24,976 pairs x 65,537 sites cost the oracle about a second per family on 16 threads.
"""
import numpy as np

A, G, C, T, N = 136, 72, 40, 24, 240
WIDTHS = (65534, 65535, 65536, 65537)
KINDS = ("plain", "runs", "hot")
N_RECORDS = 224
HALF = 32768            # first_half / second_half meet here: bit 15 of a tally
NARROW_MAX = 65535      # the last width of the packed form

# the 13 named records every kind holds (index in the set), spread so that ts_all, ts_all_copy and tv_all fall into
# different ranges of partition_square(224, 3) = rows [0, 41), [41, 95), [95, 224) or thereabouts
PLACES = {"root": 0, "all_n": 1, "ts_all": 3, "pur": 10, "pur_ts": 11, "one_site": 20, "ts_all_copy": 67, "first_half": 90,
          "pyr": 120, "pyr_ts": 150, "second_half": 180, "last_site_only": 200, "tv_all": 222}
RUN_PLACES = (30, 75, 130, 170, 210)          # kind "runs": records with long runs of N, ts_all outside them
CLADE_PLACES = (40, 41, 42, 43, 44, 45)       # kind "hot": majority records that share another base at the hot columns
ONE_SITE_AT = 40_000


def _lut(pairs):
    t = np.arange(256, dtype=np.uint8)
    for a, b in pairs:
        t[a] = b
    return t


TS = _lut(((A, G), (G, A), (C, T), (T, C)))     # the transition partner
TV = _lut(((A, C), (G, T), (C, A), (T, G)))     # a transversion, different from the transition partner too


def run_spans(L):
    """[begin, end) of the runs of N of the five run records: whole 128-site chunks by the hundred, unaligned ends, a run
    across site 32,768, one from site 0 and one to the end of the alignment (the last chunk is partial)"""
    return ((0, 20_000), (1_000, 1_000 + 128 * 130 + 17), (HALF - 5_000, HALF + 9_000), (50_000, L), (12_345, 12_345 + 128 * 9))


def boundary_alignment(L, kind="plain"):
    """(codes uint8 (224, L), names: label -> record index, or -> list of indices for "majority", "runs", "clade"; for
    kind "hot" also "hot_columns": the sorted hot sites, floor(L / 2) of them: the most the hybrid path admits)"""
    if kind not in KINDS or L <= ONE_SITE_AT + 1 or L <= HALF:
        raise ValueError((L, kind))
    rng = np.random.default_rng(20261017 + L)
    n = N_RECORDS
    R = rng.choice(np.array([A, G, C, T], np.uint8), size=L, p=[0.30, 0.20, 0.18, 0.32])
    codes = np.tile(R, (n, 1))
    special = set(PLACES.values()) | (set(RUN_PLACES) if kind == "runs" else set())
    majority = [r for r in range(n) if r not in special]
    # majority: near-copies of R, divergence 1e-3, no two of them mutated at the same site (see the module docstring)
    per = round(1e-3 * L)
    order = rng.permutation(L)
    for k, r in enumerate(majority):
        sites = order[k * per:(k + 1) * per]
        codes[r, sites] = np.where(rng.random(per) < 0.5, TS[R[sites]], TV[R[sites]])
    names = dict(PLACES)
    names["majority"] = majority
    purine = (R == A) | (R == G)
    even = (np.arange(L) & 1) == 0
    codes[names["root"]] = R
    codes[names["ts_all"]] = TS[R]
    codes[names["ts_all_copy"]] = TS[R]
    codes[names["tv_all"]] = TV[R]
    pur = np.where(purine, R, np.where(even, A, G)).astype(np.uint8)       # purines only; R where R is a purine
    pyr = np.where(~purine, R, np.where(even, C, T)).astype(np.uint8)      # pyrimidines only
    codes[names["pur"]], codes[names["pur_ts"]] = pur, TS[pur]             # tn93 count_P1 = L
    codes[names["pyr"]], codes[names["pyr_ts"]] = pyr, TS[pyr]             # tn93 count_P2 = L
    codes[names["all_n"]] = N
    codes[names["one_site"]] = N
    codes[names["one_site"], ONE_SITE_AT] = TS[R[ONE_SITE_AT]]
    codes[names["last_site_only"]] = N
    codes[names["last_site_only"], L - 1] = TS[R[L - 1]]
    codes[names["first_half"]] = R
    codes[names["first_half"], HALF:] = N
    codes[names["second_half"]] = R
    codes[names["second_half"], :HALF] = N
    if kind == "runs":
        names["runs"] = list(RUN_PLACES)
        for r, (b, e) in zip(RUN_PLACES, run_spans(L)):
            codes[r] = TS[R]
            codes[r, b:e] = N
    if kind == "hot":
        cols = np.sort(rng.choice(L, size=L // 2, replace=False))
        names["clade"] = list(CLADE_PLACES)
        names["hot_columns"] = cols
        for r in CLADE_PLACES:
            codes[r, cols] = TS[R[cols]]
    return np.ascontiguousarray(codes), names


def deviants(codes):
    """per site: how many records differ from the plurality code there (what the engine's reference sampling counts)"""
    best = np.zeros(codes.shape[1], np.int64)
    for c in (A, G, C, T, N):
        best = np.maximum(best, (codes == c).sum(axis=0))
    return codes.shape[0] - best


def extremes(names):
    """the named records in index order (the second, small set of the rectangle and stream tests)"""
    return sorted(v for k, v in names.items() if k in PLACES)


def pair_index(n, i, j):
    """canonical index of the pair (i, j), i != j, in the square's order"""
    a, b = min(i, j), max(i, j)
    return a * (2 * n - a - 1) // 2 + b - a - 1


def wide_of(L):
    """what every caller of the pair kernels derives from the width: one tally per word from 65,536 sites on"""
    return L > NARROW_MAX
