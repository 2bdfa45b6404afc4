"""The designed inputs of the dst_window_summary tests, shared by the host test (which holds the set to its design with
the oracle) and the GPU test (which runs it).  No GPU, no distance_amd."""
import numpy as np

import oracle
from helpers import KNOWN

ALL = ("n", "n_high", "raw", "jc69", "k80", "tn93")
F64 = ("raw", "jc69", "k80", "tn93")
N_CODE = 240
HOSTILE_LEN = 40


def hostile_set():
    """9 records x 40 sites.  0: all N.  1, 2: identical.  3: differs from 1 at every site.  4: differs from 1 at three of
    every four sites (p = 0.75 in every aligned 4-site window and over the whole width: jc69 +inf).  5 .. 8: uniform random
    bases, so short windows put k80 / tn93 past their logarithms' domain."""
    rng = np.random.default_rng(11)
    known = np.array(KNOWN, np.uint8)
    base = rng.integers(0, 4, HOSTILE_LEN)
    every = (base + 1 + rng.integers(0, 3, HOSTILE_LEN)) % 4          # another base at every site
    three = np.where(np.arange(HOSTILE_LEN) % 4 == 3, base, every)    # ... but the same at sites 3, 7, 11, ...
    recs = [np.full(HOSTILE_LEN, N_CODE, np.uint8), known[base], known[base], known[every], known[three]]
    recs += [known[rng.integers(0, 4, HOSTILE_LEN)] for _ in range(4)]
    return np.ascontiguousarray(np.array(recs, np.uint8))


def hostile_partner():
    """5 records of the same width for the rectangle: record 1 of the set again, and four uniform random ones"""
    rng = np.random.default_rng(12)
    known = np.array(KNOWN, np.uint8)
    return np.ascontiguousarray(np.array([hostile_set()[1]] + [known[rng.integers(0, 4, HOSTILE_LEN)] for _ in range(4)], np.uint8))


def hostile_windows():
    """the whole width, the aligned 4-site windows, an empty window, one site, and the whole width again"""
    w = [(0, HOSTILE_LEN)] + [(b, b + 4) for b in range(0, HOSTILE_LEN, 4)] + [(7, 7), (3, 4), (0, HOSTILE_LEN)]
    return np.array(w, np.uint64)


def oracle_window_payloads(measure, a, b, windows):
    """[n_windows, P] payloads in canonical order from the oracle on contiguous copies of the column slices (b None: the
    square of a), base counts by code per window.  An empty window: 0 for n / n_high, NaN for the f64 measures' 0 / 0."""
    out = []
    for lo, hi in np.asarray(windows).tolist():
        ca = np.ascontiguousarray(a[:, lo:hi])
        if hi <= lo:
            p = len(a) * (len(a) - 1) // 2 if b is None else len(a) * len(b)
            out.append(np.zeros(p) if measure in ("n", "n_high") else np.full(p, np.nan))
        elif b is None:
            out.append(oracle.all_pairs_square(measure, ca))
        else:
            out.append(oracle.all_pairs_rect(measure, ca, np.ascontiguousarray(b[:, lo:hi])).reshape(-1))
    vals = np.array(out, np.float64)
    return vals.astype(np.int64) if measure in ("n", "n_high") else vals
