"""Designed alignments for the list structures of the consensus path (dst_consensus.hip): plain numpy, no GPU.

Between an upload and a result the difference lists pass through five hand-built structures, each with a hard boundary:
  pack slot per (record, 128-site chunk)   <= 7 entries inline (kSlotEntries), else back to the planes; a chunk of N is a
                                           run chunk; the last chunk may be partial
  list piece per (record, 1,024 sites)     a thread walks 8 entries (kBucketWalk), the rest goes to a wave, 64 a round
  bucket per (panel of 2,048, site)        <= 15 entries inline (kInlineEvents), else 13 (kInlineOverflowing) and an
                                           offset; the overflow is shared over the wave 128 at a time
  batch = two rows' lists                  64 * EW entries in the register pipeline (128 / 256 / 512), slices behind it
  run records                              4 run chunks make one (kRunMin), at most n / 3 of them; MFMA tiles of 32 x 32,
                                           blocks of 128 x 128, eight mask words (256 chunks) per operand round
`census_alignment()` puts a named size on either side of each of them; `census()` counts what a code matrix holds from the
matrix alone (the sampling rule of ref_sample_kernel restated), test_list_structure_host.py asserts the counts, and
test_gpu_list_structure.py runs the sets through every path.

The census set: 4,396 records x 4,200 sites = two full panels and one of 300 records; 33 chunks, the last of 104 sites;
five site ranges.  One root sequence over A, G, C, T with the N class (N, -, ?: one nibble) at every site s % 16 == 5,
where the background records alternate N, - and ? and so make no entry.  A deviating record takes one of the 14 other
nibbles, chosen by (record + site) % 14.  Features sit on disjoint site ranges, record positions are in-panel:
  buckets   sites 0-1,023 (SIZED_SITES), one site per (panel, size), three sites with 15 / 16 / 17 in all panels at once;
            in-panel record 0 and the panel's last are members (size 1: the last alone: record-in-panel 2,047, and the
            set's last record); the reference class runs round-robin over the sites of 140 and more.  Every site of 12 and
            more of panels 1 and 2 has a probe record in panel 0 (in-panel 100, 102, ...; its neighbour 101, 103, ... has no
            entry of its own there) whose only entry in an overflowing bucket of that column panel is this one: the
            overflow its wave shares out is exactly size - 13.  Panel 0 has no lower panel and every record of it is in its
            2,048 bucket, so panel 0's exact overflows are met by the rows of the rectangle partner instead.
  slots     chunks 8-15, in-panel records 1-8: 1, 6, 7, 8, 9, 127 and 128 differences in one chunk, and a chunk of N:
            a run chunk, 120 entries (its eight N-class sites make none)
  pieces    sites 2,048-3,071, in-panel records 9-16: 7, 8, 9, 10, 71, 72, 73 and 137 entries inside the range
  batches   panel 0, entries in sites 3,072-4,095: rows (32,33) ... (48,49) whose lists sum to 127, 128, 129, 255, 256,
            257, 511, 512 and 513; rows (50,51) ... (66,67) the same without their entries at the hot columns, which the
            hybrid path leaves out of the lists.  The generator adds what the bucket feature does not already give.
  runs      panel 2, in-panel records 20-23: exactly 3 whole run chunks, exactly 4, 4 with the partial last chunk, all N
  near root in-panel record 17 of every panel is left out of the panel's all-but-one bucket: one entry.  No record can
            equal the root (an empty list): the buckets of 2,048 and 300 hold every record of their panel.  Empty lists
            are met in the run-table sets and the wide form instead.
"""
import numpy as np

A, G, C, T = 136, 72, 40, 24
N_CODES = (240, 244, 242)                       # N - ? : nibble 15
CLASS_CODE = (A, G, C, T, 240)                  # reference classes 0..4
CLASS_NIBBLE = (8, 4, 2, 1, 15)
CODE_OF_NIBBLE = {8: 136, 4: 72, 2: 40, 1: 24, 12: 192, 10: 160, 9: 144, 6: 96, 5: 80, 3: 48, 14: 224, 11: 176, 13: 208, 7: 112}

PANEL, CHUNK, RANGE, SAMPLES = 2048, 128, 1024, 512
SLOT_ENTRIES, BUCKET_WALK, INLINE, INLINE_OVER, OVF_ROUND, RUN_MIN = 7, 8, 15, 13, 128, 4
HOT_PERMILLE, MAX_DEVIATION = 50, 0.08

N_RECORDS, LENGTH = 4396, 4200
PANEL_START = (0, 2048, 4096)
PANEL_SIZE = (2048, 2048, 300)
SIZES_COMMON = (1, 12, 13, 14, 15, 16, 17, 76, 77, 78, 140, 141, 142)
SIZES = tuple(SIZES_COMMON + ((2047, 2048) if p < 2 else (299, 300)) for p in range(3))
ALL_PANELS = (15, 16, 17)                        # three sites with this size in every panel at once
SLOT_COUNTS = (1, 6, 7, 8, 9, 127, 128, "N")     # in-panel records 1..8
PIECE_COUNTS = (7, 8, 9, 10, 71, 72, 73, 137)    # in-panel records 9..16
BATCH_SUMS = (127, 128, 129, 255, 256, 257, 511, 512, 513)
NEAR_ROOT = 17
RUNS = {"three_chunks": 20, "four_chunks": 21, "four_with_partial": 22, "all_n": 23}    # in-panel, panel 2
BATCH_FIRST, BATCH_COLD_FIRST, PROBE_FIRST = 32, 50, 100
RUN_TABLE_N_RUN = (1, 32, 33, 128, 129, 233, 234)
WIDE_LENGTH = 65664


def _others():
    """OTHERS[ref nibble][k]: the 14 nibbles a record can deviate to at a site of that reference nibble"""
    t = np.zeros((16, 14), np.uint8)
    for ref in CLASS_NIBBLE:
        t[ref] = [x for x in range(1, 16) if x != ref]
    return t


OTHERS = _others()
_CODE_LUT = np.zeros(16, np.uint8)
for _nib, _code in CODE_OF_NIBBLE.items():
    _CODE_LUT[_nib] = _code


def deviate(codes, root, r, sites, shift=0):
    """record r takes, at each of `sites`, the (r + site + shift) % 14-th of the 14 nibbles that differ from the root's"""
    sites = np.asarray(sites, np.int64)
    nib = OTHERS[root[sites] >> 4, (r + sites + shift) % 14]
    codes[r, sites] = np.where(nib == 15, N_CODES[r % 3], _CODE_LUT[nib])


def sized_sites():
    """[(site, {panel: size}, reference class)]: the 48 designed bucket sites, 16 apart, N-class ones at s % 16 == 5"""
    out, big = [], 0
    for i in range(len(SIZES[0])):
        for p in range(3):
            q, size = 3 * i + p, SIZES[p][i]
            if size >= 140:
                big += 1
                cls = big % 5                     # round-robin over A, G, C, T, N
            else:
                cls = 4 if q % 5 == 4 or (p == 2 and size == 1) else q % 4    # (panel 2 holds the all-N record)
            out.append((16 * q + (5 if cls == 4 else 9), {p: size}, cls))
    for k, size in enumerate(ALL_PANELS):
        q = 3 * len(SIZES[0]) + k
        cls = (1, 4, 3)[k]
        out.append((16 * q + (5 if cls == 4 else 9), {0: size, 1: size, 2: size}, cls))
    return out


SIZED_SITES = sized_sites()
HOT_SITES = tuple(sorted(s for s, sizes, _ in SIZED_SITES if max(sizes.values()) >= 299))


def census_root():
    rng = np.random.default_rng(20261018)
    root = rng.choice(np.array([A, G, C, T], np.uint8), size=LENGTH, p=[0.30, 0.20, 0.18, 0.32])
    root[np.arange(LENGTH) % 16 == 5] = 240
    for s, _, cls in SIZED_SITES:
        assert (s % 16 == 5) == (cls == 4) and s < RANGE
        root[s] = CLASS_CODE[cls]
    return root


def background(root, n):
    """n copies of the root; at the N-class sites the records alternate N, - and ?"""
    codes = np.tile(root, (n, 1))
    ncls = np.nonzero(root >= 240)[0]
    for k in (1, 2):
        codes[np.ix_(np.arange(k, n, 3), ncls)] = N_CODES[k]
    return codes


def probes():
    """{(panel, site): record}: the probe rows of the sites of 12 and more of panels 1 and 2, in panel 0"""
    out, r = {}, PROBE_FIRST
    for s, sizes, _ in SIZED_SITES:
        if len(sizes) == 1:
            (p, size), = sizes.items()
            if p > 0 and size >= 12:
                out[(p, s)] = r
                r += 2
    return out


def reserved(p):
    """in-panel records of panel p that carry a feature of their own: not drawn as plain bucket members"""
    res = set(range(0, NEAR_ROOT + 1)) | {PANEL_SIZE[p] - 1}
    if p == 0:
        res |= set(range(BATCH_FIRST, BATCH_COLD_FIRST + 18)) | set(range(PROBE_FIRST, PROBE_FIRST + 2 * len(probes())))
    if p == 2:
        res |= set(RUNS.values())
    return res


def census_alignment():
    """(codes uint8 (4396, 4200), names): names["root"], ["sized"] = {(panel, site): size}, ["probes"] = {(panel, site):
    record}, ["slots"] = {(record, chunk): count or "N"}, ["pieces"] = {record: count in range 2}, ["batches"] /
    ["batches_cold"] = {(row, row + 1): sum}, ["runs"] = {label: record}, ["near_root"] = [records], ["hot_sites"],
    ["features"] = the sorted records that carry a feature"""
    rng = np.random.default_rng(20261027)    # (a draw that leaves every bucket of 142 and fewer at 19 sampled records or below)
    root = census_root()
    codes = background(root, N_RECORDS)
    names = {"root": root, "sized": {}, "slots": {}, "pieces": {}, "batches": {}, "batches_cold": {}, "hot_sites": HOT_SITES}
    # runs and ends first: the all-N record is a member of every bucket of its panel at a site of known reference
    P2 = PANEL_START[2]
    names["runs"] = {k: P2 + v for k, v in RUNS.items()}
    codes[names["runs"]["three_chunks"], 17 * CHUNK:20 * CHUNK] = 240
    codes[names["runs"]["four_chunks"], 20 * CHUNK:24 * CHUNK] = 244
    codes[names["runs"]["four_with_partial"], 29 * CHUNK:] = 242          # chunks 29, 30, 31 and the 104 sites of chunk 32
    codes[names["runs"]["all_n"], :] = 240
    # buckets
    for s, sizes, cls in SIZED_SITES:
        for p, size in sizes.items():
            r0, np_ = PANEL_START[p], PANEL_SIZE[p]
            forced = [k for k in range(np_) if (codes[r0 + k, s] >> 4) != (root[s] >> 4)]
            if size >= np_ - 1:
                members = [k for k in range(np_) if size == np_ or k != NEAR_ROOT]
            else:
                members = list(forced) + ([np_ - 1] if size == 1 else [0, np_ - 1])
                res = reserved(p)
                pool = [k for k in rng.permutation(np_) if k not in res and k not in members]
                members += [int(k) for k in pool[:size - len(members)]]
            assert len(set(members)) == size and set(forced) <= set(members), (s, p, size)
            for k in members:
                if k not in forced:
                    deviate(codes, root, r0 + k, [s])
            names["sized"][(p, s)] = size
    names["probes"] = probes()
    for (p, s), r in names["probes"].items():
        deviate(codes, root, r, [s])
    names["near_root"] = [PANEL_START[p] + NEAR_ROOT for p in range(3)]
    # slots: chunks 8-15
    for p in range(3):
        for f, count in enumerate(SLOT_COUNTS):
            r, chunk = PANEL_START[p] + 1 + f, 8 + (f + 3 * p) % 8
            if count == "N":
                codes[r, chunk * CHUNK:(chunk + 1) * CHUNK] = N_CODES[p]
            else:
                deviate(codes, root, r, chunk * CHUNK + np.sort(rng.permutation(CHUNK)[:count]))
            names["slots"][(r, chunk)] = count
    # pieces: range 2
    for p in range(3):
        for f, count in enumerate(PIECE_COUNTS):
            r = PANEL_START[p] + 9 + f
            deviate(codes, root, r, 2 * RANGE + np.sort(rng.permutation(RANGE)[:count]))
            names["pieces"][r] = count
    # batches: what the buckets do not already give, in range 3
    hot = np.zeros(LENGTH, bool)
    hot[list(HOT_SITES)] = True
    for first, key, cold_only in ((BATCH_FIRST, "batches", False), (BATCH_COLD_FIRST, "batches_cold", True)):
        for i, total in enumerate(BATCH_SUMS):
            for r, want in ((first + 2 * i, total // 2), (first + 2 * i + 1, total - total // 2)):
                have = (codes[r] >> 4) != (root >> 4)
                have = int((have & ~hot).sum()) if cold_only else int(have.sum())
                deviate(codes, root, r, 3 * RANGE + np.sort(rng.permutation(RANGE)[:want - have]))
            names[key][(first + 2 * i, first + 2 * i + 1)] = total
    feat = set(names["runs"].values()) | set(names["probes"].values()) | set(names["near_root"])
    feat |= {r for r, _ in names["slots"]} | set(names["pieces"]) | {r for pair in names["batches"] for r in pair}
    feat |= {r for pair in names["batches_cold"] for r in pair}
    feat |= {PANEL_START[p] for p in range(3)} | {PANEL_START[p] + PANEL_SIZE[p] - 1 for p in range(3)}
    names["features"] = sorted(feat)
    return np.ascontiguousarray(codes), names


def partner_alignment(root=None):
    """130 records of the census's width for the rectangles: record i deviates at the sized site i % 48 — its only entry in
    an overflowing bucket of any column panel, so the rows of this set are the probes of panel 0's sizes — at the sites
    of 13, 14 and 15 of panel i % 3, at six seeded sites elsewhere, and every fifth record carries a short run of N"""
    root = census_root() if root is None else root
    rng = np.random.default_rng(20261020)
    codes = background(root, 130)
    small = {p: [s for s, sizes, _ in SIZED_SITES if sizes == {p: 13} or sizes == {p: 14} or sizes == {p: 15}] for p in range(3)}
    for i in range(130):
        deviate(codes, root, i, [SIZED_SITES[i % 48][0]] + small[i % 3], shift=3)
        deviate(codes, root, i, RANGE + np.sort(rng.permutation(LENGTH - RANGE)[:6]), shift=3)
        if i % 5 == 0:
            a = int(rng.integers(RANGE, LENGTH - 300))
            codes[i, a:a + 40 + i] = N_CODES[i % 3]
    return np.ascontiguousarray(codes)


def wide_form(codes, names):
    """the census's feature records and 600 background records, padded with constant columns to 65,664 sites (513
    chunks: one tally per word, the wide kernels)"""
    keep = sorted(set(names["features"]) | {int(r) for r in np.linspace(200, N_RECORDS - 2, 600).astype(int)})
    out = np.full((len(keep), WIDE_LENGTH), A, np.uint8)
    out[:, :LENGTH] = codes[keep]
    return out, keep


def run_table_alignment(n_run, n=700, L=1280, n_class_every=2, seed=5):
    """The run-table sets.  The first n_run records carry 4 run chunks from chunk (37 record) % (chunks - 3) on — staggered, so
    that two records' masks overlap in 0 to 4 chunks — the others are near-copies of the root (3 substitutions per 1,000
    sites; every third record is the root itself: an empty list).  Every n_class_every-th site is of the N class: the fused
    preparation keeps its lists only while the 512 sampled records deviate at no more than 8 % of the sites, and 233
    records with 512 sites of N in 1,280 would be 13 %; with every other site of the N class a run chunk is 64 entries and
    the sum stays below the gate."""
    rng = np.random.default_rng(20261021 + seed)
    root = rng.choice(np.array([A, G, C, T], np.uint8), size=L)
    root[np.arange(L) % n_class_every == n_class_every - 1] = 240
    codes = background(root, n)
    nch = -(-L // CHUNK)
    known = np.nonzero(root < 240)[0]
    for r in range(n):
        if r % 3:
            deviate(codes, root, r, np.sort(rng.choice(known, size=max(1, round(3e-3 * L)), replace=False)))
    for r in range(n_run):
        c = (37 * r) % (nch - 3) if r < n_run - 1 else nch - 4     # the last run record reaches the last chunk
        codes[r, c * CHUNK:(c + 4) * CHUNK] = N_CODES[r % 3]
    return np.ascontiguousarray(codes)


# ---------------------------------------------------------------------------------------------------------------------
# the census: what a code matrix holds, from the matrix alone
# ---------------------------------------------------------------------------------------------------------------------
def sampled_records(n):
    """ref_sample_kernel's sample: record floor(k n / 512) for k < 512 (every record while n <= 512)"""
    return np.arange(n) if n <= SAMPLES else (np.arange(SAMPLES, dtype=np.int64) * n) // SAMPLES


def sampled_reference(codes):
    """(reference nibble per site, sampled deviants per site, hot flags): the plurality over A, G, C, T and the N class among
    the sampled records, ties to the first in that order (strict >); hot: deviants * 1000 > samples * 50"""
    nib = codes[sampled_records(len(codes))] >> 4
    counts = np.stack([(nib == x).sum(axis=0) for x in CLASS_NIBBLE])
    best, cls = counts[0].copy(), np.zeros(codes.shape[1], np.int64)
    for k in range(1, 5):
        better = counts[k] > best
        best[better], cls[better] = counts[k][better], k
    dev = len(nib) - best
    return np.array(CLASS_NIBBLE, np.uint8)[cls], dev, dev * 1000 > len(nib) * HOT_PERMILLE


def census(codes, ref_nibble=None):
    """dict of counts, from the code matrix and the reference nibbles (default: the sampled reference's):
    diff (n, L) bool; per_chunk (n, chunks); per_range (n, ranges); bucket (panels, L); length (n,); run_chunks (n,):
    whole chunks of nibble 15, sites past the end counting as N, like on the device"""
    n, L = codes.shape
    if ref_nibble is None:
        ref_nibble = sampled_reference(codes)[0]
    nib = codes >> 4
    diff = nib != ref_nibble[None, :]
    nch, nrg, npan = -(-L // CHUNK), -(-L // RANGE), -(-n // PANEL)
    pad = np.zeros((n, nch * CHUNK), bool)
    pad[:, :L] = diff
    isn = np.ones((n, nch * CHUNK), bool)
    isn[:, :L] = nib == 15
    rpad = np.zeros((n, nrg * RANGE), bool)
    rpad[:, :L] = diff
    return {"diff": diff, "per_chunk": pad.reshape(n, nch, CHUNK).sum(axis=2), "per_range": rpad.reshape(n, nrg, RANGE).sum(axis=2),
            "bucket": np.stack([diff[p * PANEL:(p + 1) * PANEL].sum(axis=0) for p in range(npan)]),
            "length": diff.sum(axis=1), "run_chunks": isn.reshape(n, nch, CHUNK).all(axis=2).sum(axis=1)}


def run_record_count(run_chunks):
    """how many run records the fused preparation makes: the records of kRunMin run chunks and more, none when they are
    more than a third of the set"""
    k, n = int((np.asarray(run_chunks) >= RUN_MIN).sum()), len(run_chunks)
    return k if k <= n // 3 else 0


def batch_sums(length, row_begin, row_end, rows_per_tile, last_column=None):
    """the entries of every batch (two rows from the tile's first row on) of a launch over rows [row_begin, row_end)"""
    out = []
    end = row_end if last_column is None else min(row_end, last_column)
    for i0 in range(row_begin, end, rows_per_tile):
        i1 = min(end, i0 + rows_per_tile)
        out += [int(length[q:min(q + 2, i1)].sum()) for q in range(i0, i1, 2)]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the per-site table of the four tally families, for the host test's tie to the oracle
# ---------------------------------------------------------------------------------------------------------------------
def tally_tables():
    """{family: int (256, 256, width)}: what one site of codes (a, b) adds to each tally, written from the definitions:
    a site counts as compared when both codes are the same known base, or when they share no nibble bit (a difference)"""
    pur, pyr, known = (136, 72, 192), (40, 24, 48), (136, 72, 40, 24)
    valid = sorted(CODE_OF_NIBBLE.values()) + list(N_CODES)
    t = {"n_high": np.zeros((256, 256, 1), np.int64), "raw": np.zeros((256, 256, 2), np.int64),
         "k80": np.zeros((256, 256, 3), np.int64), "tn93": np.zeros((256, 256, 4), np.int64)}
    for a in valid:
        for b in valid:
            same, differ = a == b and a in known, ((a >> 4) & (b >> 4)) == 0
            t["n_high"][a, b, 0] = differ
            t["raw"][a, b] = (differ, same or differ)
            if same:
                t["k80"][a, b, 0] = t["tn93"][a, b, 0] = 1
            elif differ:
                ts = (a in pur and b in pur) or (a in pyr and b in pyr)
                tv = (a in pur and b in pyr) or (a in pyr and b in pur)
                t["k80"][a, b] = (ts or tv, ts, tv)
                if a in known and b in known:
                    t["tn93"][a, b] = (1, 1, {a, b} == {A, G}, {a, b} == {C, T})
    return t


def table_tallies(table, q, t):
    return table[q, t].sum(axis=0)
