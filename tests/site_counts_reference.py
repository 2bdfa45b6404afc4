"""The definition of dst_site_counts / dst_site_stats restated: the counts by numpy from the code matrix (the classes from
the code's high nibble alone), the window statistics with plain Python loops in the operation order the header fixes, and
the text of the CLI's two modes from both."""
import numpy as np

NONE = 0xFFFFFFFF
CLASSES = 5
# high nibble -> class: A (1000), T (0001), G (0100), C (0010) in the library's {A,T,G,C} order; 4: two or three bases;
# -1: N, - and ? (1111), in no class.  No code has an empty high nibble.
NIBBLE_CLASS = np.full(16, 4, np.int64)
NIBBLE_CLASS[0b1000], NIBBLE_CLASS[0b0001], NIBBLE_CLASS[0b0100], NIBBLE_CLASS[0b0010] = 0, 1, 2, 3
NIBBLE_CLASS[0b1111] = NIBBLE_CLASS[0] = -1


def labels_u32(groups, n):
    """None: one group of every record; else integer labels with -1 as DST_GROUP_NONE"""
    if groups is None:
        return np.zeros(n, np.uint32)
    g = np.asarray(groups).astype(np.int64)
    return np.where(g == -1, NONE, g).astype(np.uint32)


def group_sizes(groups, n, n_groups):
    g = labels_u32(groups, n)
    return np.array([int((g == a).sum()) for a in range(n_groups)], np.uint64)


def site_counts(codes, groups=None, n_groups=1, begin=0, end=None):
    """(end - begin, n_groups, 5) uint32"""
    codes = np.asarray(codes, np.uint8)
    n, length = codes.shape
    end = length if end is None else end
    g = labels_u32(groups, n)
    cls = NIBBLE_CLASS[codes[:, begin:end] >> 4]            # (n, sites)
    out = np.zeros((end - begin, n_groups, CLASSES), np.uint32)
    for a in range(n_groups):
        rows = cls[g == a]
        for k in range(CLASSES):
            out[:, a, k] = (rows == k).sum(axis=0)
    return out


def site_stats(counts, windows, sizes, site_begin=0):
    """dict of (n_windows, G) arrays, every floating-point operation in the header's order"""
    counts = np.asarray(counts)
    G = counts.shape[1]
    nw = len(windows)
    out = {k: np.zeros((nw, G), np.uint64) for k in ("records", "sites", "called", "segregating")}
    out["theta_sum"], out["pi_sum"] = np.zeros((nw, G)), np.zeros((nw, G))
    harmonic = [0.0]
    for w, (wb, we) in enumerate(windows):
        wb, we = int(wb), int(we)
        if not (site_begin <= wb <= we <= site_begin + counts.shape[0]):
            raise ValueError(f"window {w} outside the counted sites")
        for g in range(G):
            called = seg = 0
            theta = pi = 0.0
            for s in range(wb, we):
                a, t, gg, c = (int(x) for x in counts[s - site_begin, g, :4])
                m = a + t + gg + c
                if m < 2:
                    continue
                called += 1
                d = a * t + a * gg + a * c + t * gg + t * c + gg * c
                pi = pi + float(d) / float(m * (m - 1) // 2)
                if (a != 0) + (t != 0) + (gg != 0) + (c != 0) < 2:
                    continue
                seg += 1
                while len(harmonic) < m:
                    harmonic.append(harmonic[-1] + 1.0 / float(len(harmonic)))
                theta = theta + 1.0 / harmonic[m - 1]
            out["records"][w, g], out["sites"][w, g] = int(sizes[g]), we - wb
            out["called"][w, g], out["segregating"][w, g] = called, seg
            out["theta_sum"][w, g], out["pi_sum"][w, g] = theta, pi
    return out


def counts_text(counts, names, sizes):
    """`distance --site-counts`: the file order of a line's bases is A C G T"""
    lines = ["site\tgroup\trecords\tA\tC\tG\tT\tambiguous\tmissing"]
    for s in range(counts.shape[0]):
        for g, name in enumerate(names):
            a, t, gg, c, amb = (int(x) for x in counts[s, g])
            lines.append(f"{s + 1}\t{name}\t{int(sizes[g])}\t{a}\t{c}\t{gg}\t{t}\t{amb}\t{int(sizes[g]) - a - t - gg - c - amb}")
    return "\n".join(lines) + "\n"


def stats_text(stats, window_fields, names, fmt):
    """`distance --window-site-stats`; window_fields[w] = the plain windows run's first three fields, fmt = the mean
    formatter of --summary (a float -> its text)"""
    lines = ["window\tstart\tend\tgroup\trecords\tsites\tcalled\tsegregating\ttheta_w\tpi"]
    for w, first in enumerate(window_fields):
        for g, name in enumerate(names):
            called = int(stats["called"][w, g])
            theta = fmt(stats["theta_sum"][w, g] / called) if called else "NaN"
            pi = fmt(stats["pi_sum"][w, g] / called) if called else "NaN"
            lines.append(f"{first}\t{name}\t{int(stats['records'][w, g])}\t{int(stats['sites'][w, g])}\t{called}\t"
                         f"{int(stats['segregating'][w, g])}\t{theta}\t{pi}")
    return "\n".join(lines) + "\n"
