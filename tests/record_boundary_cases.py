"""A designed set past 65,535 records and 2^32 canonical pair offsets, with exact closed-form answers: plain numpy, no GPU.

92,700 records have 4,296,598,650 pairs, more than 2^32 = 4,294,967,296: row 65,536 starts at canonical offset
3,927,670,784 and row 90,894 is the first whose start is at or above 2^32.  Brute force over 4.3e9 pairs is out of reach
on the CPU, so the set is built so that every whole-set answer has a cheap exact reference.

Records.  Record r carries a distinct 20-bit word w_r (drawn without replacement, so the input order is not word order).
  * site b < 20 holds one of two letters by bit b of the word: even b A (bit 0) or G (bit 1), so a difference there is a
    transition; odd b A or C, a transversion.  n(i, j) = popcount(w_i ^ w_j), its even bits the transitions (tn93's
    purine transitions P1; there is no T in the set), its odd bits the transversions.
  * sites 20..39 are A, except that record r has N in its last r % 3 sites: comparable(i, j) = 40 - max(i % 3, j % 3), and
    raw = n / comparable takes three denominators whose values interleave (2/40 < 2/39 < 2/38 < 3/40 ...).  raw is the
    IEEE quotient, so numpy's quotient is its exact reference.

References, all exact:
  links(T <= 2 ...)   flip 1, 2, ... bits of every word and look the result up in a 2^20 table
  clusters            union-find over the distance-1 links, labels the smallest record of each cluster
  mst                 mst_reference.kruskal_edges over the links of radius 1, then 2, ... until the forest is complete: an
                      edge of a larger distance comes later in the (distance, i, j) order than every edge seen, and a
                      complete forest takes no further edge, so the rest of the order is never needed
  histogram           the integer Walsh-Hadamard autocorrelation of the words' indicator, binned by popcount
  per-record sum      sum over the bits b of the number of records whose bit b differs from the record's own
  one row             popcount of the row's word against all n
  a column window   the same forms with the word masked to the window's bits and 40 replaced by the window's comparable
                      sites (window_tallies, window_values, window_base_counts)
test_record_boundary_host.py holds this design to the oracle on picked rows; test_gpu_record_boundary.py and
test_gpu_cli_record_boundary.py run the engine and the command-line tool on it, test_gpu_record_boundary_windows.py the
windowed operations, the pair lists and the window-closest stream, the latter also on tall_set(): 524,289 records of the
same design, nine more than the 65,535 rows of one launch grid hold at eight records each."""
import functools
import itertools

import numpy as np

from mst_reference import kruskal_edges

A, G, C, N = 136, 72, 40, 240
N_RECORDS = 92_700
BITS = 20
LENGTH = 40
SEED = 2026
TWO32 = 1 << 32
GRID_ROWS = 65_535                      # the most rows of one launch grid
FIRST_ROW_PAST_2_32 = 90_894            # the first row whose canonical start is >= 2^32 (asserted by the host test)
FIXED_ROWS = (0, 65_534, 65_535, 65_536, 65_537, 90_893, 90_894, N_RECORDS - 2, N_RECORDS - 1)
N_PICKED = 300
EVEN = sum(1 << b for b in range(0, BITS, 2))
ODD = sum(1 << b for b in range(1, BITS, 2))
POP = np.zeros(1 << BITS, np.uint8)     # popcount of every 20-bit word
for _b in range(BITS):
    POP += ((np.arange(1 << BITS, dtype=np.uint32) >> _b) & 1).astype(np.uint8)
LETTER = {A: "A", G: "G", C: "C", N: "N"}
# item 3j: the greedy cut at this bound gives two slabs, the second of more than 65,535 rows (asserted by the host test)
TWO_SLAB_MAX_PAIRS = 2_149_000_000


def row_start(n, i):
    """canonical offset of pair (i, i + 1): Python integers or int64 arrays"""
    return i * (2 * n - i - 1) // 2


def canon(n, i, j):
    """canonical ordinal of the pairs (i < j), int64"""
    i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
    return i * (2 * n - i - 1) // 2 + (j - i - 1)


def cut_row_slabs(n, max_pairs):
    """The engine's greedy cut of the square's rows restated: [(rb, re, first_pair, pairs)], every slab at most max_pairs
    pairs but at least one row, slabs without pairs dropped."""
    start = row_start(n, np.arange(n + 1, dtype=np.int64))
    start[n] = start[n - 1]   # (row n - 1 has no pairs)
    slabs, rb = [], 0
    while rb < n:
        re = int(np.searchsorted(start, start[rb] + max_pairs, side="right")) - 1
        re = min(max(re, rb + 1), n)
        if re == n - 1:       # the last row adds nothing: the greedy loop takes it too
            re = n
        pairs = int(start[re] - start[rb])
        if pairs:
            slabs.append((rb, re, int(start[rb]), pairs))
        rb = re
    return slabs


class RecordSet:
    """words uint32[n], codes uint8[n, 40], and the table word -> record (-1: no such record)"""

    def __init__(self, n=N_RECORDS, seed=SEED):
        rng = np.random.default_rng(seed)
        self.n = n
        self.words = rng.permutation(1 << BITS)[:n].astype(np.uint32)
        self.table = np.full(1 << BITS, -1, np.int64)
        self.table[self.words] = np.arange(n)
        codes = np.full((n, LENGTH), A, np.uint8)
        for b in range(BITS):
            codes[:, b] = np.where((self.words >> b) & 1, G if b % 2 == 0 else C, A)
        r = np.arange(n)
        codes[r % 3 >= 1, LENGTH - 1] = N
        codes[r % 3 == 2, LENGTH - 2] = N
        self.codes = codes
        seeded = rng.choice(n, N_PICKED, replace=False)
        self.picked = np.unique(np.concatenate([np.array(FIXED_ROWS), seeded[:N_PICKED - len(FIXED_ROWS)]])).astype(np.int64)
        self.rng_seed = seed

    # ---- per pair ---------------------------------------------------------------------------------------------------
    def xor(self, i, j):
        return self.words[np.asarray(i, np.int64)] ^ self.words[np.asarray(j, np.int64)]

    def comparable(self, i, j):
        return LENGTH - np.maximum(np.asarray(i, np.int64) % 3, np.asarray(j, np.int64) % 3)

    def tallies(self, measure, i, j):
        """the measure's DST_OUT_TALLY words of the pairs (i, j), int64 (len, width)"""
        x = self.xor(i, j)
        d, comp = POP[x].astype(np.int64), self.comparable(i, j)
        ts, tv = POP[x & EVEN].astype(np.int64), POP[x & ODD].astype(np.int64)
        if measure in ("n", "n_high"):
            return d[:, None]
        if measure in ("raw", "jc69"):
            return np.stack([d, comp], axis=1)
        if measure == "k80":
            return np.stack([comp, ts, tv], axis=1)
        if measure == "tn93":
            return np.stack([comp, d, ts, np.zeros_like(d)], axis=1)
        raise ValueError(measure)

    def values(self, measure, i, j):
        """the DST_OUT_DISTANCE payloads of n, n_high (int64) or raw (float64, the IEEE quotient) of the pairs (i, j)"""
        d = POP[self.xor(i, j)].astype(np.int64)
        if measure in ("n", "n_high"):
            return d
        if measure == "raw":
            return d.astype(np.float64) / self.comparable(i, j).astype(np.float64)
        raise ValueError(measure)

    def base_counts(self):
        """{A, T, G, C} of every record, uint32 (n, 4)"""
        g, c = POP[self.words & EVEN].astype(np.int64), POP[self.words & ODD].astype(np.int64)
        a = LENGTH - np.arange(self.n) % 3 - g - c
        return np.stack([a, np.zeros_like(a), g, c], axis=1).astype(np.uint32)

    def row(self, measure, i):
        """record i against all n records (itself included: 0)"""
        return self.values(measure, np.full(self.n, i), np.arange(self.n))

    # ---- per pair, inside a column window [b, e) of the 40 sites -----------------------------------------------------
    def window_comparable(self, i, j, b, e):
        """the sites of [b, e) at which neither record holds N: e - b less site 39 when max(i % 3, j % 3) >= 1 and
        site 38 when it is 2, each only when the window holds it (i == j: the record against itself)"""
        worst = np.maximum(np.asarray(i, np.int64) % 3, np.asarray(j, np.int64) % 3)
        gone = ((worst >= 1) & (b <= LENGTH - 1 < e)).astype(np.int64) + ((worst == 2) & (b <= LENGTH - 2 < e))
        return max(e - b, 0) - gone

    def window_tallies(self, measure, i, j, b, e):
        """tallies() of the pairs (i, j) on the sets cut to the columns [b, e): the xor word masked to the window's bits,
        LENGTH replaced by the window's comparable sites; an empty window gives zeros"""
        x = self.xor(i, j) & window_mask(b, e)
        d, comp = POP[x].astype(np.int64), self.window_comparable(i, j, b, e)
        ts, tv = POP[x & EVEN].astype(np.int64), POP[x & ODD].astype(np.int64)
        if measure in ("n", "n_high"):
            return d[:, None]
        if measure in ("raw", "jc69"):
            return np.stack([d, comp], axis=1)
        if measure == "k80":
            return np.stack([comp, ts, tv], axis=1)
        if measure == "tn93":
            return np.stack([comp, d, ts, np.zeros_like(d)], axis=1)
        raise ValueError(measure)

    def window_values(self, measure, i, j, b, e):
        """values() of the pairs (i, j) on the sets cut to the columns [b, e); raw is NaN where no site is comparable"""
        d = POP[self.xor(i, j) & window_mask(b, e)].astype(np.int64)
        if measure in ("n", "n_high"):
            return d
        if measure == "raw":
            with np.errstate(invalid="ignore", divide="ignore"):
                return d.astype(np.float64) / self.window_comparable(i, j, b, e).astype(np.float64)
        raise ValueError(measure)

    def window_base_counts(self, b, e):
        """{A, T, G, C} of every record inside the columns [b, e), uint32 (n, 4)"""
        mask = window_mask(b, e)
        g, c = POP[self.words & EVEN & mask].astype(np.int64), POP[self.words & ODD & mask].astype(np.int64)
        r = np.arange(self.n)
        a = self.window_comparable(r, r, b, e) - g - c
        return np.stack([a, np.zeros_like(a), g, c], axis=1).astype(np.uint32)

    # ---- whole set --------------------------------------------------------------------------------------------------
    @functools.lru_cache(maxsize=None)
    def links_at(self, d):
        """(i, j) int64 of every pair i < j at distance exactly d, in canonical order"""
        idx = np.arange(self.n, dtype=np.int64)
        parts_i, parts_j = [], []
        for bits in itertools.combinations(range(BITS), d):
            mask = np.uint32(sum(1 << b for b in bits))
            partner = self.table[self.words ^ mask]
            keep = partner > idx
            parts_i.append(idx[keep])
            parts_j.append(partner[keep])
        i, j = np.concatenate(parts_i), np.concatenate(parts_j)
        order = np.argsort(i * self.n + j, kind="stable")
        return i[order], j[order]

    def links_within(self, radius):
        """(i, j, distance) int64 of every pair i < j at distance <= radius (>= 1: the words are distinct), canonical order"""
        parts = [self.links_at(d) for d in range(1, radius + 1)]
        i = np.concatenate([p[0] for p in parts])
        j = np.concatenate([p[1] for p in parts])
        d = np.concatenate([np.full(len(p[0]), k + 1, np.int64) for k, p in enumerate(parts)])
        order = np.argsort(i * self.n + j, kind="stable")
        return i[order], j[order], d[order]

    def within(self, i, j):
        """partners per record of the link list (i, j)"""
        return (np.bincount(i, minlength=self.n) + np.bincount(j, minlength=self.n)).astype(np.uint32)

    @functools.lru_cache(maxsize=None)
    def clusters(self, radius=1):
        """labels uint32[n] of the single-linkage clusters at T = radius: the smallest record of each (radius 0: every
        record its own, the words are distinct)"""
        parent = np.arange(self.n, dtype=np.int64)
        if radius >= 1:
            a, b, _ = self.links_within(radius)
            while True:
                while True:
                    nxt = parent[parent]
                    if np.array_equal(nxt, parent):
                        break
                    parent = nxt
                ra, rb = parent[a], parent[b]
                cross = ra != rb
                if not cross.any():
                    break
                lo, hi = np.minimum(ra[cross], rb[cross]), np.maximum(ra[cross], rb[cross])
                np.minimum.at(parent, hi, lo)
                a, b = a[cross], b[cross]
        return parent.astype(np.uint32)

    @functools.lru_cache(maxsize=None)
    def mst(self):
        """(edges int64[n - 1, 2], values int64[n - 1], the radius at which the forest became complete): Kruskal in the
        (distance, i, j) order over the links of radius 1, 2, ... (see the module docstring).  Links inside one cluster of
        the smaller radii are left out before the loop: Kruskal would reject every one of them."""
        edges, vals, state, radius = [], [], None, 0
        while sum(len(e) for e in edges) < self.n - 1:
            radius += 1
            i, j = self.links_at(radius)
            if radius > 1:
                lab = self.clusters(radius - 1)
                cross = lab[i] != lab[j]
                i, j = i[cross], j[cross]
            taken, state = kruskal_edges(self.n, i, j, state)
            edges.append(np.stack([i[taken], j[taken]], axis=1))
            vals.append(np.full(len(taken), radius, np.int64))
        return np.concatenate(edges), np.concatenate(vals), radius

    @functools.lru_cache(maxsize=None)
    def histogram(self):
        """uint64[21]: the pairs i < j at every distance 0 .. 20, from the Walsh-Hadamard autocorrelation"""
        auto = xor_counts(self.words, self.words)   # ordered pairs (i, j) with w_i ^ w_j = x
        assert int(auto[0]) == self.n
        auto[0] = 0
        by_distance = np.array([int(auto[POP == d].sum()) for d in range(BITS + 1)], np.int64)
        assert (by_distance % 2 == 0).all()
        return (by_distance // 2).astype(np.uint64)

    def sums(self):
        """int64[n]: every record's sum of n over its n - 1 partners"""
        out = np.zeros(self.n, np.int64)
        for b in range(BITS):
            bit = ((self.words >> b) & 1).astype(np.int64)
            ones = int(bit.sum())
            out += np.where(bit == 1, self.n - ones, ones)
        return out

    # ---- ids and FASTA --------------------------------------------------------------------------------------------
    def ids(self):
        """ids of mixed length (2 to 17 characters)"""
        prefix = ("s", "rec_", "sample-long.")
        return [f"{prefix[r % 3]}{r}" for r in range(self.n)]

    def write_fasta(self, path):
        lut = np.zeros(256, np.uint8)
        for code, letter in LETTER.items():
            lut[code] = ord(letter)
        rows = lut[self.codes].view(f"S{LENGTH}").ravel()
        with open(path, "wb") as fh:
            fh.write(b"".join(b">%s\n%s\n" % (i.encode(), s) for i, s in zip(self.ids(), rows)))
        return self.ids()

    def site_field(self, i, j):
        """the --sites field of pair (i, j): X<pos>Y per differing site, ascending, 1-based; "." without one"""
        x = int(self.words[i] ^ self.words[j])
        out = []
        for b in range(BITS):
            if x >> b & 1:
                out.append(f"{LETTER[int(self.codes[i, b])]}{b + 1}{LETTER[int(self.codes[j, b])]}")
        return ",".join(out) if out else "."


def xor_counts(words_a, words_b):
    """int64[2^20]: for every x the pairs (a of words_a, b of words_b) with a ^ b = x (both lists of distinct words), as the
    Walsh-Hadamard transform of the product of the two indicators' transforms; every intermediate is below 2^63"""
    f, g = np.zeros(1 << BITS, np.int64), np.zeros(1 << BITS, np.int64)
    f[words_a] = 1
    g[words_b] = 1
    return wht(wht(f) * wht(g)) >> BITS


def wht(a):
    """the unnormalised Walsh-Hadamard transform of an int64 vector of 2^k entries"""
    a = a.copy()
    h = 1
    while h < len(a):
        v = a.reshape(-1, 2, h)
        lo, hi = v[:, 0, :].copy(), v[:, 1, :].copy()
        v[:, 0, :] = lo + hi
        v[:, 1, :] = lo - hi
        h *= 2
    return a


@functools.lru_cache(maxsize=None)
def record_set():
    """the set of the module docstring, built once per process"""
    return RecordSet()


# ---- windows, named pairs and window streams (test_gpu_record_boundary_windows.py) ---------------------------------------
# the whole width, the varying half, an inner cut, the N tail, the last two sites (almost all ties), one site, an empty window
WINDOWS = ((0, 40), (0, 20), (3, 17), (20, 40), (38, 40), (0, 1), (39, 39))
NEAREST_WINDOWS = ((0, 40), (3, 17), (38, 40))
WIN_ROWS = 8                                # row records of one block of the window sweep
TALL_RECORDS = WIN_ROWS * GRID_ROWS + 9     # 524,289: one window launch of more than 65,535 row tiles, a second grid
TALL_SEED = 2027
TALL_ROW_BEGIN = 3                          # a row range whose second grid begins off a multiple of 8
WINDOW_NEAREST_PAIRS = 1 << 25              # pair-windows of a slab of dst_nearest_windows unless the caller says otherwise
WINDOW_NEAREST_LISTS_MAX = 1 << 31          # (row, window) lists of one slab
FIRST_RECT_ROW_PAST_2_32 = 46_332           # the first row of the 92,700 x 92,700 rectangle whose start i n is >= 2^32


def window_mask(b, e):
    """bits b .. min(e, 20) - 1 of a word: the varying sites inside the window [b, e)"""
    return np.uint32(sum(1 << s for s in range(b, min(e, BITS))))


def cut_window_slabs(n_rows, n_windows, n_cols, max_entries=0):
    """The engine's cut of the (row, window) lists of dst_nearest_windows or of a window-closest stream's batch restated:
    (rows, windows) of one slab.  Whole row ranges of all the windows while a row's windows fit the budget, else at most
    eight rows of a range of windows."""
    budget = min(max_entries, 1 << 40) if max_entries else WINDOW_NEAREST_PAIRS
    lists = min(max(budget // n_cols, 1), WINDOW_NEAREST_LISTS_MAX)
    if lists >= n_windows:
        return min(lists // n_windows, n_rows), n_windows
    rows = min(lists, WIN_ROWS, n_rows)
    return rows, lists // rows


def second_grid_first_row(row_begin, row_end):
    """the first row of the window sweep's second launch grid over rows [row_begin, row_end), or None when one grid holds
    all the row tiles"""
    tiles = -(-(row_end - row_begin) // WIN_ROWS)
    return row_begin + GRID_ROWS * WIN_ROWS if tiles > GRID_ROWS else None


@functools.lru_cache(maxsize=None)
def tall_set():
    """524,289 records of the same design (2^20 distinct words suffice), built once per process"""
    return RecordSet(n=TALL_RECORDS, seed=TALL_SEED)


def tall_columns(n=TALL_RECORDS):
    """the five records of the tall set that are the columns (or the streamed batch): first, last, three in between"""
    return np.array([0, WIN_ROWS * GRID_ROWS - 1, WIN_ROWS * GRID_ROWS, n - 2, n - 1], np.int64)


@functools.lru_cache(maxsize=None)
def boundary_pairs(n=N_RECORDS, seed=31):
    """(row, col) int64 of the square list of run_pairs: the pairs at the boundaries and two diagonal entries, about 2,000
    seeded pairs whose canonical rows lie in [65,530, 65,545) and [90,890, n - 1) (so the sweep runs a handful of slabs), each
    in both orders, shuffled, with repeats"""
    F = FIRST_ROW_PAST_2_32
    fixed = [(65_535, 65_536), (65_536, n - 1), (F - 1, F), (F, n - 1), (n - 2, n - 1), (65_536, 65_536), (n - 1, n - 1)]
    rng = np.random.default_rng(seed)
    i = np.concatenate([rng.integers(65_530, 65_545, 1_000), rng.integers(90_890, n - 1, 1_000)])
    j = i + 1 + (rng.random(2_000) * (n - 1 - i)).astype(np.int64)
    i, j = np.concatenate([[p[0] for p in fixed], i]), np.concatenate([[p[1] for p in fixed], j])
    row, col = np.concatenate([i, j, i[:5]]), np.concatenate([j, i, j[:5]])
    order = rng.permutation(len(row))
    return row[order].astype(np.int64), col[order].astype(np.int64)


@functools.lru_cache(maxsize=None)
def boundary_rect_pairs(n=N_RECORDS, seed=32):
    """(row, col) int64 of the rectangle list of run_pairs on 92,700 x 92,700: the two entries either side of position 2^32,
    two diagonal entries, and about 1,000 seeded pairs of the rows [46,334, 46,340), [65,530, 65,545) and [n - 10, n), all
    past 2^32; shuffled, with repeats"""
    fixed = [(FIRST_RECT_ROW_PAST_2_32 - 1, TWO32 - (FIRST_RECT_ROW_PAST_2_32 - 1) * n - 1),
             (FIRST_RECT_ROW_PAST_2_32 - 1, TWO32 - (FIRST_RECT_ROW_PAST_2_32 - 1) * n),
             (FIRST_RECT_ROW_PAST_2_32, 0), (65_535, n - 1), (65_536, 0), (65_536, 65_536), (n - 1, n - 1), (n - 1, 0)]
    rng = np.random.default_rng(seed)
    i = rng.choice(np.concatenate([np.arange(46_334, 46_340), np.arange(65_530, 65_545), np.arange(n - 10, n)]), 1_000)
    j = rng.integers(0, n, 1_000)
    row, col = np.concatenate([[p[0] for p in fixed], i, i[:5]]), np.concatenate([[p[1] for p in fixed], j, j[:5]])
    order = rng.permutation(len(row))
    return row[order].astype(np.int64), col[order].astype(np.int64)


def touched_slabs(n, max_pairs, row, col):
    """the slabs of cut_row_slabs(n, max_pairs) that hold a listed pair off the diagonal, by its canonical row"""
    slabs = cut_row_slabs(n, max_pairs)
    lo = np.minimum(row, col)[row != col]
    begins = np.array([s[0] for s in slabs])
    hit = np.unique(np.searchsorted(begins, lo, side="right") - 1)
    assert all(slabs[k][0] <= r < slabs[k][1] for k, r in zip(np.searchsorted(begins, lo, side="right") - 1, lo))
    return [slabs[k] for k in hit]


def max_pairs_cutting_in(n, row_lo, row_hi, lo=1 << 25, hi=1 << 26):
    """the smallest slab bound lo + 9973 k below hi whose greedy cut begins a slab at a row in [row_lo, row_hi]"""
    start = row_start(n, np.arange(n + 1, dtype=np.int64))
    for max_pairs in range(lo, hi, 9973):
        rb = 0
        while rb < row_lo:
            re = int(np.searchsorted(start, start[rb] + max_pairs, side="right")) - 1
            rb = max(re, rb + 1)
        if rb <= row_hi:
            return max_pairs
    raise ValueError("no bound in the range cuts there")
