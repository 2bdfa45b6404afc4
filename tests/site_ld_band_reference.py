"""The definitions of dst_ld_band / dst_site_ld_band / dst_site_ld_links_band / dst_site_ld_decay restated: the band by plain
loops over the list, the tiles as the set of (p // 64, q // 64) of its pairs, the bins with Python integers, q = rint(r2 x
2^30) as a Python integer (float x 2^30 is exact, round() ties to even), and the text of `distance --ld R2 --ld-decay W`."""
import math

import numpy as np

from site_ld_reference import finalize_one, listed_sites, pair_index

TILE = 64
SCALE_BITS = 30


def band_rows(sites, max_gap):
    """row_end[p]: the first position past p whose gap to p is above max_gap, by brute force"""
    s = [int(x) for x in sites]
    out = []
    for p in range(len(s)):
        e = p + 1
        while e < len(s) and s[e] - s[p] <= max_gap:
            e += 1
        out.append(e)
    return np.array(out, np.uint32)


def band_pairs(sites, max_gap, row_begin=0, row_end=None):
    """the pairs (p, q) of the band in canonical order, row_begin <= p < row_end: every pair of the list is looked at"""
    s = [int(x) for x in sites]
    return [(p, q) for p, q in pair_index(len(s), row_begin, row_end) if s[q] - s[p] <= max_gap]


def band_tiles(sites, max_gap):
    return len({(p // TILE, q // TILE) for p, q in band_pairs(sites, max_gap)})


def band_mask(sites, max_gap, row_begin=0, row_end=None):
    """bool over the canonical pairs of the row range: the pair is in the band"""
    s = [int(x) for x in sites]
    return np.array([s[q] - s[p] <= max_gap for p, q in pair_index(len(s), row_begin, row_end)], bool)


def links_in_band(sites, max_gap, pos_i, pos_j, tallies):
    """site_ld_links' arrays filtered by the gap"""
    s = np.asarray(sites, np.int64)
    keep = (s[np.asarray(pos_j, np.int64)] - s[np.asarray(pos_i, np.int64)]) <= max_gap
    return pos_i[keep], pos_j[keep], tallies[keep]


def q_of(r2):
    """rint(r2 x 2^30), ties to even, as a Python integer"""
    return round(float(r2) * float(1 << SCALE_BITS))


def decay_pairs(sites, width, bins):
    s = [int(x) for x in sites]
    out = [0] * bins
    for p, q in pair_index(len(s)):
        b = (s[q] - s[p]) // width
        if b < bins:
            out[b] += 1
    return np.array(out, np.uint64)


def decay(sites, tallies, width, bins, min_r2, r2=None):
    """the curve from the tallies of EVERY pair of the list in canonical order: {"pairs", "defined", "links"} as uint64, "q"
    as Python integers, "r2_sum" = float(q) x 2^-30.  r2: the pairs' r2 when the caller has them (ld_finalize's), else
    finalize_one's."""
    s = [int(x) for x in sites]
    pairs, defined, links, q = [0] * bins, [0] * bins, [0] * bins, [0] * bins
    for e, (p, j) in enumerate(pair_index(len(s))):
        b = (s[j] - s[p]) // width
        if b >= bins:
            continue
        pairs[b] += 1
        v = float(r2[e]) if r2 is not None else finalize_one(*tallies[e])[0]
        if math.isnan(v):
            continue
        defined[b] += 1
        links[b] += v >= min_r2
        q[b] += q_of(v)
    return {"pairs": np.array(pairs, np.uint64), "defined": np.array(defined, np.uint64), "links": np.array(links, np.uint64), "q": q,
            "r2_sum": np.array([float(x) * 2.0 ** -SCALE_BITS for x in q], np.float64)}


def same_curve(got, want):
    """the engine's dict against decay()'s, bit for bit"""
    return (all(np.array_equal(got[k], want[k]) and got[k].dtype == np.uint64 for k in ("pairs", "defined", "links"))
            and np.array_equal(np.asarray(got["r2_sum"]).view(np.uint64), want["r2_sum"].view(np.uint64)))


def decay_text(codes, tallies_of, min_r2, width, bins, min_count=1, groups=None, names=("all",), fmt=None):
    """`distance --ld R2 --ld-decay W --ld-bins B`: tallies_of(sites, alleles, g) -> the tallies of every pair of the group's
    list in canonical order; fmt = the mean formatter of --summary"""
    lines = ["group\tgap\tpairs\tdefined\tlinked\tmean_r2"]
    for g, name in enumerate(names):
        sites, allele = listed_sites(codes, groups, g, min_count)
        if len(sites) < 2:
            continue
        c = decay(sites, tallies_of(sites, allele, g), width, bins, min_r2)
        for b in range(bins):
            d = int(c["defined"][b])
            mean = "NaN" if d == 0 else fmt(float(c["r2_sum"][b]) / float(d))
            lines.append(f"{name}\t{b * width}\t{int(c['pairs'][b])}\t{d}\t{int(c['links'][b])}\t{mean}")
    return "\n".join(lines) + "\n"
