"""The definition of dst_site_ld / dst_site_ld_links / dst_ld_finalize / dst_site_major restated: the tallies by plain loops
over the code matrix (the sets from the code's high nibble alone), the three statistics with Python integers and floats in
the operation order the header fixes, the major allele from dst_site_counts' entries, and the text of `distance --ld`."""
import math

import numpy as np

from site_counts_reference import NIBBLE_CLASS, site_counts

NONE = 0xFFFFFFFF
NAN_BITS = 0x7FF8000000000000
LETTERS = "ATGC"   # the library's class order


def taking_part(n, groups=None, which=0):
    """bool[n]: the records with groups[x] == which (-1: DST_GROUP_NONE); None: every record"""
    if groups is None:
        return np.ones(n, bool)
    g = np.asarray(groups).astype(np.int64)
    return np.where(g == -1, NONE, g) == which


def site_sets(codes, sites, alleles, groups=None, which=0):
    """(C, M): bool[S, n]"""
    codes = np.asarray(codes, np.uint8)
    part = taking_part(codes.shape[0], groups, which)
    C = np.zeros((len(sites), codes.shape[0]), bool)
    M = np.zeros_like(C)
    for p, (s, ref) in enumerate(zip(sites, alleles)):
        cls = NIBBLE_CLASS[codes[:, int(s)] >> 4]          # 0..3: one base; 4: two or three; -1: N, - and ?
        C[p] = part & (cls >= 0) & (cls <= 3)
        M[p] = C[p] & (cls != int(ref))
    return C, M


def tallies(codes, sites, alleles, groups=None, which=0, row_begin=0, row_end=None):
    """uint32[P, 4]: {m, a, b, c} of the pairs p < q, row_begin <= p < row_end, in canonical order"""
    S = len(sites)
    row_end = S if row_end is None else row_end
    C, M = site_sets(codes, sites, alleles, groups, which)
    out = []
    for p in range(row_begin, row_end):
        for q in range(p + 1, S):
            out.append((int((C[p] & C[q]).sum()), int((M[p] & C[q]).sum()), int((C[p] & M[q]).sum()), int((M[p] & M[q]).sum())))
    return np.array(out, np.uint32).reshape(len(out), 4)


def tallies_by_products(codes, sites, alleles, groups=None, which=0):
    """the same tallies of every pair from four integer matrix products (exact), for lists too long for the loops above;
    the tests compare the two on short lists"""
    C, M = site_sets(codes, sites, alleles, groups, which)
    Ci, Mi = C.astype(np.int64), M.astype(np.int64)
    i, j = np.triu_indices(len(sites), 1)   # row-major: the canonical order
    return np.stack([(Ci @ Ci.T)[i, j], (Mi @ Ci.T)[i, j], (Ci @ Mi.T)[i, j], (Mi @ Mi.T)[i, j]], axis=1).astype(np.uint32)


def pair_index(S, row_begin=0, row_end=None):
    row_end = S if row_end is None else row_end
    return [(p, q) for p in range(row_begin, row_end) for q in range(p + 1, S)]


def finalize_one(m, a, b, c):
    """(r2, D, Dprime) of one pair: Python integers are exact, float(int) is the one correctly rounded conversion, and each
    * and / on floats is one IEEE operation"""
    m, a, b, c = int(m), int(a), int(b), int(c)
    num = m * c - a * b
    A, B = a * (m - a), b * (m - b)
    nan = math.nan
    d = float(num) / float(m * m) if m else nan
    if A == 0 or B == 0:
        return nan, d, nan
    r2 = (float(num) * float(num)) / (float(A) * float(B))
    x = min(a * (m - b), (m - a) * b) if num >= 0 else min(a * b, (m - a) * (m - b))
    return r2, d, float(num) / float(x)


def finalize(t):
    t = np.asarray(t).reshape(-1, 4)
    out = {k: np.zeros(len(t)) for k in ("r2", "d", "dprime")}
    for e, row in enumerate(t):
        out["r2"][e], out["d"][e], out["dprime"][e] = finalize_one(*row)
    return out


def same_bits(got, want):
    """float arrays equal bit for bit, every NaN the quiet NaN 0x7FF8000000000000"""
    g, w = np.asarray(got, np.float64).view(np.uint64), np.asarray(want, np.float64).view(np.uint64).copy()
    w[np.isnan(np.asarray(want, np.float64))] = NAN_BITS
    return g.shape == w.shape and bool((g == w).all())


def site_major(counts, g=0):
    """(allele uint8, major uint32, other uint32) per site: the largest of the four base counts, ties to the smallest class"""
    counts = np.asarray(counts)
    allele, major, other = [], [], []
    for s in range(counts.shape[0]):
        c = [int(x) for x in counts[s, g, :4]]
        best = 0
        for k in range(1, 4):
            if c[k] > c[best]:
                best = k
        allele.append(best), major.append(c[best]), other.append(sum(c) - c[best])
    return np.array(allele, np.uint8), np.array(major, np.uint32), np.array(other, np.uint32)


def links(codes, sites, alleles, min_r2, groups=None, which=0):
    """(pos_i, pos_j, tallies) of the pairs whose r2 is not NaN and >= min_r2, in canonical order"""
    t = tallies(codes, sites, alleles, groups, which)
    keep = [e for e, row in enumerate(t) if not math.isnan(finalize_one(*row)[0]) and finalize_one(*row)[0] >= min_r2]
    idx = pair_index(len(sites))
    return (np.array([idx[e][0] for e in keep], np.uint32), np.array([idx[e][1] for e in keep], np.uint32),
            t[keep].reshape(len(keep), 4))


def listed_sites(codes, groups, which, min_count):
    """`distance --ld`'s choice for one group: the sites whose major and other counts are both >= min_count, their alleles"""
    member = None if groups is None else np.where(taking_part(len(codes), groups, which), 0, -1)
    allele, major, other = site_major(site_counts(codes, member, 1), 0)
    keep = [s for s in range(codes.shape[1]) if major[s] >= min_count and other[s] >= min_count]
    return np.array(keep, np.uint32), allele[keep]


def ld_text(codes, min_r2, min_count=1, groups=None, names=("all",), fmt=None):
    """`distance --ld R2 [--ld-min-count C] [--ld-groups FILE]`: fmt = the mean formatter of --summary (a float -> its text)"""
    codes = np.asarray(codes, np.uint8)
    lines = ["site1\tsite2\tgroup\tmajor1\tmajor2\tcalled\tminor1\tminor2\tboth\tr2\tD\tDprime"]
    for g, name in enumerate(names):
        sites, allele = listed_sites(codes, groups, g, min_count)
        if len(sites) < 2:
            continue
        pi, pj, t = links(codes, sites, allele, min_r2, groups, g)
        for i, j, row in zip(pi, pj, t):
            r2, d, dp = finalize_one(*row)
            m, a, b, c = (int(x) for x in row)
            lines.append(f"{int(sites[i]) + 1}\t{int(sites[j]) + 1}\t{name}\t{LETTERS[allele[i]]}\t{LETTERS[allele[j]]}\t{m}\t{a}\t{b}\t{c}\t"
                         + "\t".join("NaN" if math.isnan(v) else fmt(v) for v in (r2, d, dp)))
    return "\n".join(lines) + "\n"
