"""Designed alignments for the shared preparation (dst_upload_shared, dst_shared.cpp): plain numpy, no GPU.

A shared upload cuts the records into shares of rmax = ceil(n / world) rounded up to 256, lists each share into an
exchange block of fixed entry capacity, and rebuilds the range marks of every record's list (range_marks_kernel: "the
index of the first entry at or beyond site g * 1,024") from the exchanged lists, 64 entries a round.  The sets here put a
named size on either side of each of those:
  cut_set()        1,100 x 4,200: list lengths 0 ... 193 around the 64-lane rounds, lists that skip ranges, lie in the
                   last range only (site 4,199 among them) or in range 0 only, the slot switch, a chunk of N, a piece of
                   73 — on the records either side of every rank cut of world 2 ... 5 and once inside a share
  fit_sets()       512 x 4,200 for world 2: rank 0's share lists exactly 40,960 entries (the first upload's block
                   capacity, 256 * 96 + 16,384) and 40,961
  cooled_census()  the census of list_structure_cases.py without its panel-wide buckets (the hot columns): everything
                   else of it on the shared path; the census itself is the `hot_columns` fallback
  wide_cut_set()   the wide form (65,664 sites: 65 ranges) plus three records for the trailing marks
  diverse_set()    600 x 1,000 at 30 % divergence: past the 8 % gate, the `diverse` fallback
  small_set(n)     n = 2, 257, 300 at 300 sites: every record sampled, shares of one record and of none
test_shared_structure_host.py holds every one of them to its design from the code matrix alone."""
import numpy as np

import list_structure_cases as ls
from list_structure_cases import A, C, G, T, CHUNK, RANGE, N_CODES, background, deviate

SHARE_ROUND, FIRST_PER_RECORD, FIRST_EXTRA = 256, 96, 16384      # shared_layout and dst_shared.cpp's first capacity

CUT_N, CUT_L = 1100, 4200
CUT_RECORDS = (255, 256, 511, 512, 767, 768, 1023, 1024, 1099)
LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 193)
# (kind, parameter): what a feature record's list is
FEATURES = tuple(("length", k) for k in LENGTHS) + (("ranges_0_and_4", None), ("range_4_only", None), ("range_0_only", None),
                                                    ("chunk", 7), ("chunk", 8), ("chunk", 9), ("chunk_of_n", None), ("piece", 73))
# the features of the records at the cuts: the 64-lane rounds and the range skips sit on both sides of every cut
CUT_FEATURES = {255: ("length", 64), 256: ("length", 65), 511: ("length", 0), 512: ("length", 63), 767: ("length", 128),
                768: ("length", 129), 1023: ("ranges_0_and_4", None), 1024: ("range_4_only", None), 1099: ("length", 193)}
MID_FIRST, MID_STEP = 100, 60                       # mid-share records 100, 160, ... 1,060: one per feature
FEATURE_CHUNK, N_CHUNK, PIECE_RANGE = 12, 20, 2

FIT_N, FIT_L, FIT_WORLD = 512, 4200, 2
FIT_CAPACITY = 256 * FIRST_PER_RECORD + FIRST_EXTRA      # 40,960
FIT_PER_RECORD, FIT_LIGHT = 160, 3

SMALL_L = 300


def share_size(n, world):
    """records per rank: ceil(n / world) rounded up to a multiple of 256 (shared_layout)"""
    return -(-(-(-n // world)) // SHARE_ROUND) * SHARE_ROUND


def shares(n, world):
    """[(begin, end)] of every rank (dst_shared_range restated)"""
    rmax = share_size(n, world)
    return [(min(n, k * rmax), min(n, (k + 1) * rmax)) for k in range(world)]


def first_capacity(n, world):
    """the entry capacity of a block at the first shared upload of a slot"""
    return (share_size(n, world) * FIRST_PER_RECORD + FIRST_EXTRA + 3) & ~3


def next_capacity(biggest):
    """... and at the next one, from the largest block the previous exchange reported"""
    return (biggest + biggest // 4 + 4096 + 3) & ~3


def _feature(codes, root, r, feature, rng):
    kind, k = feature
    L = codes.shape[1]
    last = (L - 1) // RANGE
    if kind == "length":                            # from five entries on, one of them in every range
        spread = [int(rng.integers(g * RANGE, min((g + 1) * RANGE, L))) for g in range(last + 1)] if k >= last + 1 else []
        rest = [int(x) for x in rng.permutation(L) if int(x) not in spread]
        sites = np.array(spread + rest[:k - len(spread)], np.int64)
    elif kind == "ranges_0_and_4":                  # one entry (the first of range 4) is the mark of ranges 1-4
        sites = np.concatenate([rng.permutation(RANGE)[:5], last * RANGE + rng.permutation(L - last * RANGE)[:3]])
    elif kind == "range_4_only":                    # inside the 104-site tail, the last site among them
        sites = np.concatenate([last * RANGE + rng.permutation(L - 1 - last * RANGE)[:5], [L - 1]])
    elif kind == "range_0_only":
        sites = rng.permutation(RANGE)[:9]
    elif kind == "chunk":
        sites = FEATURE_CHUNK * CHUNK + rng.permutation(CHUNK)[:k]
    elif kind == "piece":
        sites = PIECE_RANGE * RANGE + rng.permutation(RANGE)[:k]
    elif kind == "chunk_of_n":
        codes[r, N_CHUNK * CHUNK:(N_CHUNK + 1) * CHUNK] = N_CODES[r % 3]
        return
    else:
        raise ValueError(kind)
    deviate(codes, root, r, np.sort(sites))


def cut_set():
    """(codes uint8 (1100, 4200), names): names["root"], ["features"] = {record: (kind, parameter)}, ["mid"] = {feature:
    record}.  Every record without a feature carries three seeded substitutions, so that no two rows are alike."""
    rng = np.random.default_rng(20261101)
    root = ls.census_root()
    codes = background(root, CUT_N)
    features = dict(CUT_FEATURES)
    mid = {}
    for i, f in enumerate(FEATURES):
        mid[f] = MID_FIRST + MID_STEP * i
        features[mid[f]] = f
    for r in range(CUT_N):
        if r in features:
            _feature(codes, root, r, features[r], rng)
        else:
            deviate(codes, root, r, np.sort(rng.permutation(CUT_L)[:3]), shift=1)
    return np.ascontiguousarray(codes), {"root": root, "features": features, "mid": mid}


def fit_sets():
    """(fits, over, names): two sets of 512 x 4,200 that differ in one code of record 255.  Every record of rank 0's share
    (world 2: records 0-255) deviates at 160 seeded sites: 40,960 entries, the first upload's capacity to the entry; `over`
    has one more.  Rank 1's records carry three entries each."""
    rng = np.random.default_rng(20261102)
    root = ls.census_root()
    codes = background(root, FIT_N)
    order = rng.permutation(FIT_L)        # the heavy records walk one seeded order of the sites: 9 or 10 of them at a site
    for r in range(FIT_N):
        if r < 256:
            sites = order[(r * FIT_PER_RECORD + np.arange(FIT_PER_RECORD)) % FIT_L]
        else:
            sites = rng.permutation(FIT_L)[:FIT_LIGHT]
        deviate(codes, root, r, np.sort(sites))
    over = codes.copy()
    free = np.nonzero((over[255] >> 4) == (root >> 4))[0]
    extra = int(free[len(free) // 2])
    deviate(over, root, 255, [extra])
    return np.ascontiguousarray(codes), np.ascontiguousarray(over), {"root": root, "extra_site": extra}


def cooled_census():
    """census_alignment() with the columns of its panel-wide buckets back at the background (but for the record that is
    all N, which stays so): (codes, names), names as the census's with "hot_sites" = ()"""
    codes, names = ls.census_alignment()
    plain = background(names["root"], ls.N_RECORDS)
    keep = np.ones(ls.N_RECORDS, bool)
    keep[names["runs"]["all_n"]] = False
    cols = np.array(ls.HOT_SITES)
    codes[np.ix_(keep, cols)] = plain[np.ix_(keep, cols)]
    names = dict(names, cooled_sites=ls.HOT_SITES, hot_sites=())
    return np.ascontiguousarray(codes), names


def wide_root(root):
    out = np.full(ls.WIDE_LENGTH, A, np.uint8)
    out[:len(root)] = root
    return out


def wide_cut_set():
    """(codes (k + 3, 65664), names): wide_form of the cooled census and three records behind it — "beyond" with its only
    entry at a site >= 65,536 (range 64), "range_0" with entries in range 0 only (64 trailing marks), "ranges_63_64" with
    one entry in each of the last two ranges"""
    codes, names = cooled_census()
    wide, keep = ls.wide_form(codes, names)
    root = wide_root(names["root"])
    extra = background(root, 3)
    k = len(keep)
    out = np.concatenate([wide, extra])
    added = {"beyond": k, "range_0": k + 1, "ranges_63_64": k + 2}
    deviate(out, root, added["beyond"], [65600])
    deviate(out, root, added["range_0"], [3, 200, 201, 640, 1023])
    deviate(out, root, added["ranges_63_64"], [63 * RANGE + 10, 64 * RANGE + 4])
    return np.ascontiguousarray(out), {"root": root, "keep": keep, "added": added}


def diverse_set():
    """600 x 1,000 over A, G, C, T, every code off the root with probability 0.3"""
    rng = np.random.default_rng(20261103)
    bases = np.array([A, G, C, T], np.uint8)
    root = rng.integers(0, 4, 1000)
    pick = np.tile(root, (600, 1))
    off = rng.random((600, 1000)) < 0.3
    pick[off] = (pick[off] + rng.integers(1, 4, int(off.sum()))) % 4
    return np.ascontiguousarray(bases[pick])


def small_set(n):
    """n records of 300 sites: the census root's first 300 sites, record r with r % 5 seeded entries (every fifth record
    is the root: an empty list), and a short run of N in every seventh"""
    rng = np.random.default_rng(20261104 + n)
    root = ls.census_root()[:SMALL_L].copy()
    codes = background(root, n)
    for r in range(n):
        deviate(codes, root, r, np.sort(rng.permutation(SMALL_L)[:r % 5]))
        if r % 7 == 3:
            codes[r, 40 + r % 100:60 + r % 100] = N_CODES[r % 3]
    return np.ascontiguousarray(codes)


# ---------------------------------------------------------------------------------------------------------------------
# what the exchange must rebuild, from the code matrix alone
# ---------------------------------------------------------------------------------------------------------------------
def share_totals(length, n, world):
    """list entries of every rank's share"""
    return [int(length[b:e].sum()) for b, e in shares(n, world)]


def hot_weight(dev, hot, samples):
    """dst_shared.cpp's `hot_columns` figure: the sum over the hot sites of (sampled deviants)^2, over samples^2"""
    return float((dev[hot].astype(np.int64) ** 2).sum()) / float(samples * samples)


def range_marks(diff_row, n_ranges):
    """mark g of a record: the index, in its ascending list, of the first entry at or beyond site g * 1,024"""
    sites = np.nonzero(diff_row)[0]
    return np.searchsorted(sites, np.arange(n_ranges) * RANGE, side="left")


def range_marks_by_rounds(diff_row, n_ranges):
    """the same marks the way range_marks_kernel finds them: 64 entries a round, an entry is the mark of every multiple
    that lies behind its predecessor's site and not behind its own, the multiples behind the last entry get the length"""
    sites = np.nonzero(diff_row)[0]
    marks = np.full(n_ranges, -1, np.int64)
    nxt = 0
    for base in range(0, len(sites), 64):
        mine = np.minimum(sites[base:base + 64] // RANGE + 1, n_ranges)
        before = np.maximum(np.concatenate([[nxt], mine[:-1]]), nxt)
        for lane in range(len(mine)):
            marks[before[lane]:mine[lane]] = base + lane
        nxt = max(nxt, int(mine[-1]))
    marks[nxt:] = len(sites)
    return marks
