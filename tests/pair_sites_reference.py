"""The definition of dst_pair_sites restated in numpy, straight from the Paradis code bytes and independent of the library.

a, b = the high nibbles of the row and the column record's codes at a site (A 8, G 4, C 2, T 1, N / - / ? 15).  The site is
listed for a measure when it adds 1 to the measure's difference tally:
  n, n_high, raw, jc69   (a & b) == 0
  k80                    ... and each of a, b is purine-class {8, 4, 12} or pyrimidine-class {2, 1, 3}
  tn93                   ... and both a and b are one of {8, 4, 2, 1}"""
import numpy as np

LETTER = {8: "A", 4: "G", 2: "C", 1: "T", 12: "R", 10: "M", 9: "W", 6: "S", 5: "K", 3: "Y", 14: "V", 11: "H", 13: "D", 7: "B"}
# which DST_OUT_TALLY words add up to the difference tally
DIFF_WORDS = {"n": (0,), "n_high": (0,), "raw": (0,), "jc69": (0,), "k80": (1, 2), "tn93": (1,)}


def listed(measure, a, b):
    """a, b: arrays of high nibbles; the boolean array of listed sites"""
    a, b = np.asarray(a, np.uint8), np.asarray(b, np.uint8)
    out = (a & b) == 0
    if measure == "k80":
        cls = lambda x: np.isin(x, (8, 4, 12)) | np.isin(x, (2, 1, 3))
        out &= cls(a) & cls(b)
    elif measure == "tn93":
        one = lambda x: np.isin(x, (8, 4, 2, 1))
        out &= one(a) & one(b)
    elif measure not in ("n", "n_high", "raw", "jc69"):
        raise ValueError(measure)
    return out


def expected(measure, row_codes, col_codes, row, col, block=1 << 16):
    """(offsets uint64[n_pairs + 1], sites uint32[total], bases uint8[total]) of pairs (row_codes[row[e]], col_codes[col[e]])"""
    row, col = np.asarray(row, np.int64), np.asarray(col, np.int64)
    rn, cn = row_codes >> 4, col_codes >> 4
    counts, sites, bases = [np.zeros(0, np.int64)], [np.zeros(0, np.uint32)], [np.zeros(0, np.uint8)]
    for e0 in range(0, len(row), block):
        a, b = rn[row[e0:e0 + block]], cn[col[e0:e0 + block]]
        m = listed(measure, a, b)
        counts.append(m.sum(axis=1, dtype=np.int64))
        sites.append(np.nonzero(m)[1].astype(np.uint32))   # (row-major: pair after pair, ascending sites)
        bases.append((a << 4 | b)[m].astype(np.uint8))
    offsets = np.concatenate([[0], np.cumsum(np.concatenate(counts))]).astype(np.uint64)
    return offsets, np.concatenate(sites), np.concatenate(bases)


def render(sites, bases, lo, hi):
    """the CLI's fourth field of one pair: X<pos>Y, comma-separated, pos 1-based; "." when there is none"""
    lo, hi = int(lo), int(hi)
    if lo == hi:
        return "."
    return ",".join(f"{LETTER[int(bases[k]) >> 4]}{int(sites[k]) + 1}{LETTER[int(bases[k]) & 15]}" for k in range(lo, hi))
