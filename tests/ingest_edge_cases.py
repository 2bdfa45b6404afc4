"""The designed cases of the ingest edges (no GPU): what test_ingest_edges_host.py holds to itself and to the oracle, and
what test_gpu_ingest_edges.py / test_gpu_cli_ingest_edges.py send through pack_kernel / pack_chunk, pack_stream_kernel and
pack_nibbles_kernel (distance_amd/csrc/dst_kernels.hip).

One property: a result depends on the bytes inside the rows, on all of them, and on nothing else.  So every case puts its
rows (helpers.uniform_codes: all 17 codes at every site) into a buffer whose every other byte is hostile:

  "invalid"  0x00, no code and no nibble: a read past a row must surface as "invalid nucleotide code";
  "valid"    seeded known bases (136, 72, 40, 24; nibbles 8, 4, 2, 1), different from row to row: a read past a row
             raises nothing and moves tallies and base counts.

The widths put the row's end at every position of the kernels' last words: L mod 8 (a 32-bit word of nibbles) and L mod 4
(a word of code bytes) on both sides of a multiple of the 128-site chunk.  The models at the end of the file say which of
pack_chunk's three load paths a (record, chunk) takes and how many sites of a last word lie inside the row, so that the
host test can assert the coverage from the case list itself."""
import functools

import numpy as np

from helpers import KNOWN, uniform_codes

CHUNK = 128            # kChunkSites
BLOCK = 256            # records of a block, along the set, in all three kernels
ALL = ("n", "n_high", "raw", "jc69", "k80", "tn93")
DISTANCES = ("n", "n_high", "raw", "tn93")      # held to the oracle's values; jc69 / k80 through their tallies
FILLS = ("invalid", "valid")
WIRES = ("codes", "nibbles")
BASE_NIBBLES = (8, 4, 2, 1)

WIDTHS = tuple(sorted(set(range(1, 18)) | {31, 32, 33, 63, 64, 65} | set(range(120, 137)) | set(range(248, 265))
                      | {383, 384, 385}))
CODE_WIDTHS = WIDTHS + (1023, 1024, 1025, 1026, 1027, 1039)     # ... and pack_stream_kernel's first span
BATCHES = (1, 2, 3)
BLOCK_EDGE_COUNTS = (255, 256, 257)
BLOCK_EDGE_WIDTHS = (1, 127, 129, 257)
N_LOADED = 40
# upload_device: every L mod 4 on both sides of 128 k, and the first span's edge
DEVICE_WIDTHS = (1, 2, 3, 5, 124, 125, 126, 127, 128, 129, 130, 131, 132, 252, 253, 254, 255, 256, 257, 258, 259, 260, 1023, 1024, 1025, 1026,
                 1027)
DEVICE_COUNTS = (1, 2, 3, 257)
SLACK = CHUNK + 4      # hostile bytes behind the last row: a whole chunk and a word

# (width, records) -> seed, where the default seed's rows do not meet test_ingest_edges_host's "the tests can fail" condition
SEEDS = {(4, 1): [7001, 4, 1, 9], (4, 2): [7001, 4, 2, 1], (4, 3): [7001, 4, 3, 2]}   # (tn93 is rarely finite on 4 sites)


def widths(wire):
    return CODE_WIDTHS if wire == "codes" else WIDTHS


def batch_counts(L):
    return BATCHES + (BLOCK_EDGE_COUNTS if L in BLOCK_EDGE_WIDTHS else ())


def pitch_of(L, wire="codes"):
    """rows of a stream's ring slot, and of the staging buffer of a host upload (codes), are this far apart"""
    if wire == "nibbles":
        return max(((L + CHUNK - 1) // CHUNK * (CHUNK // 2) + 127) // 128 * 128, 128)
    return max((L + CHUNK - 1) // CHUNK * CHUNK, CHUNK)


@functools.lru_cache(maxsize=None)
def case_rows(L, n):
    codes = uniform_codes(n, L, SEEDS.get((L, n), [7001, L, n]))
    codes.setflags(write=False)
    return codes


@functools.lru_cache(maxsize=None)
def loaded_set(L):
    codes = uniform_codes(N_LOADED, L, [2003, L])
    codes.setflags(write=False)
    return codes


# ---- hostile bytes ------------------------------------------------------------------------------------------------
def fill_bytes(fill, shape, seed, wire="codes"):
    """bytes for everything that is no row: 0x00, or known bases (both nibbles a base on the nibble wire)"""
    if fill == "invalid":
        return np.zeros(shape, np.uint8)
    assert fill == "valid", fill
    rng = np.random.default_rng([9001, int(seed)])
    if wire == "codes":
        return rng.choice(np.array(KNOWN, np.uint8), size=shape)
    nib = np.array(BASE_NIBBLES, np.uint8)
    return rng.choice(nib, size=shape) | (rng.choice(nib, size=shape) << 4)


def pad_nibble(fill, seed):
    """the unused high nibble of an odd width's last byte: 0 (no nibble) or a base"""
    return 0 if fill == "invalid" else BASE_NIBBLES[int(seed) % 4]


def to_wire(codes, wire, pad=15):
    """the rows as they cross the link: code bytes, or high nibbles two to a byte (site 2k in the low nibble)"""
    if wire == "codes":
        return np.ascontiguousarray(codes)
    hi = np.asarray(codes, np.uint8) >> 4
    if hi.shape[1] % 2:
        hi = np.concatenate([hi, np.full((hi.shape[0], 1), pad, np.uint8)], axis=1)
    return hi[:, 0::2] | (hi[:, 1::2] << 4)


def from_nibbles(wire_rows, L):
    """the sites' nibbles back out of wire bytes (numpy, nothing of the engine's)"""
    w = np.asarray(wire_rows, np.uint8)
    nib = np.empty((w.shape[0], 2 * w.shape[1]), np.uint8)
    nib[:, 0::2] = w & 15
    nib[:, 1::2] = w >> 4
    return nib[:, :L]


def hostile_buffer(codes, offset, stride, fill, seed):
    """a flat buffer with row r of `codes` at offset + r * stride and hostile bytes everywhere else, SLACK of them behind
    the last row; returns (buffer, the (n, L) view of the rows in it)"""
    n, L = codes.shape
    assert stride >= L and offset >= 0
    buf = fill_bytes(fill, offset + (n - 1) * stride + L + SLACK, seed)
    view = np.lib.stride_tricks.as_strided(buf[offset:], shape=(n, L), strides=(stride, 1))
    view[...] = codes
    return buf, view


def row_mask(n, L, offset, stride, size):
    """which bytes of such a buffer belong to a row"""
    mask = np.zeros(size, bool)
    for r in range(n):
        mask[offset + r * stride:offset + r * stride + L] = True
    return mask


def hostile_slot(slot, wire_rows, fill, seed, wire):
    """fill a stream slot's whole (max_records, pitch) view — the tails of the rows and the records behind the batch —
    with hostile bytes, then write the batch's wire rows"""
    slot[...] = fill_bytes(fill, slot.shape, seed, wire)
    slot[:wire_rows.shape[0], :wire_rows.shape[1]] = wire_rows


def primer(n, pitch, seed):
    """an upload that leaves known bases, different from row to row, in the staging buffer's row tails"""
    return fill_bytes("valid", (n, pitch), seed)


# ---- where a device upload's rows lie: (offset, stride) ------------------------------------------------------------
def layouts(L):
    """every offset mod 4 x every stride mod 4 (with a gap of 4..7 bytes between rows), rows back to back, offsets 4, 8
    and 16, every row on a 16-byte boundary, and that stride plus 1"""
    out = []
    for o in range(4):
        for r in range(4):
            out.append((o, L + (r - L) % 4 + 4))
    out.append((0, L))
    out += [(o, L + 5) for o in (4, 8, 16)]
    s16 = (L + 16) // 16 * 16
    out += [(0, s16), (0, s16 + 1)]
    return out


# ---- plants for the invalid-code report ----------------------------------------------------------------------------
def plants(L, n, wire="codes"):
    """lists of (record, site) to make invalid together; named() says which one the report must name"""
    sites = sorted({0, L - 1} | {s for s in (CHUNK - 1, CHUNK) if s < L})     # (L - 1 of an odd L: the lone low nibble)
    records = sorted({0, n - 1} | {r for r in (BLOCK - 1, BLOCK) if r < n})
    single = [(r, s) for r in records for s in sites]
    out = [[p] for p in single]
    if len(single) > 1:
        out.append([single[-1], single[0]])                        # the set's two corners
        out.append([(records[-1], sites[0]), (records[0], sites[-1])])   # later record first site, earlier record last site
        out.append([(records[-1], sites[-1]), (records[-1], sites[0])])  # one record, two sites
    return out


def named(plant, L):
    return min(plant, key=lambda p: p[0] * L + p[1])


def planted(codes, plant, wire, pad=15):
    """the wire rows with every (record, site) of the plant made invalid: a byte no code has, or nibble 0"""
    bad = np.array(codes, np.uint8)
    if wire == "codes":
        for r, s in plant:
            bad[r, s] = 0x89 if (r + s) % 2 else 0x07
        return bad
    w = to_wire(bad, wire, pad)
    for r, s in plant:
        w[r, s // 2] &= 0xF0 if s % 2 == 0 else 0x0F
    return w


# ---- models of the kernels' switches -------------------------------------------------------------------------------
def code_load_path(base_mod16, stride, n, L, s, c):
    """pack_chunk's choice for (record s, chunk c) of an n x L matrix whose first byte lies at base_mod16 (mod 16)"""
    rows16 = base_mod16 % 16 == 0 and stride % 16 == 0
    start4 = base_mod16 % 4 == 0
    site0 = c * CHUNK
    if rows16 and site0 + CHUNK <= L:
        return "fast"
    if s * stride + site0 + CHUNK + 4 <= (n - 1) * stride + L and (s > 0 or c > 0 or start4):
        return "words"
    return "bytes"


def last_word_keeps(L, sites_per_word):
    """sites inside the row of every word of the row's last chunk that reaches past its end: 0 .. sites_per_word - 1"""
    c = (L - 1) // CHUNK
    return {max(L - first, 0) for first in range(c * CHUNK, (c + 1) * CHUNK, sites_per_word) if first + sites_per_word > L}


def code_keeps_by_path(base_mod16, stride, n, L):
    """{path: set of keep} over the records' last chunks"""
    out = {}
    c = (L - 1) // CHUNK
    for s in range(n):
        path = code_load_path(base_mod16, stride, n, L, s, c)
        if path != "fast":
            out.setdefault(path, set()).update(last_word_keeps(L, 4))
    return out


# ---- what a wrong mask would read ----------------------------------------------------------------------------------
def extend(codes, tails, upto):
    """the rows with the bytes that follow them in memory appended, up to site `upto` (exclusive)"""
    n, L = codes.shape
    upto = max(upto, L)
    return np.concatenate([np.asarray(codes), np.asarray(tails)[:, :upto - L]], axis=1)


def round_up(L, k):
    return (L + k - 1) // k * k


def buffer_tails(buf, n, L, offset, stride):
    """the SLACK bytes behind every row of a hostile_buffer (the next row's bytes among them where rows lie closer)"""
    return np.stack([buf[offset + r * stride + L:offset + r * stride + L + SLACK] for r in range(n)])


def nibble_tail_codes(slot_rows, L):
    """the sites behind L of a nibble slot's rows, as the codes their nibbles stand for (a base nibble b: b << 4 | 8)"""
    w = np.asarray(slot_rows, np.uint8)
    nib = np.empty((w.shape[0], 2 * w.shape[1]), np.uint8)
    nib[:, 0::2] = w & 15
    nib[:, 1::2] = w >> 4
    tail = nib[:, L:]
    return (tail << 4) | np.where(np.isin(tail, BASE_NIBBLES), 8, 0).astype(np.uint8)
