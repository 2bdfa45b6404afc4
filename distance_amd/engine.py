"""Host-side mirror of the reference's run() boundary over the C ABI.

`Engine` owns one dst_ctx (one GPU).  Naming follows the reference: `upload` replaces
Setup.loaded_fastas (src/lib.rs:133-144), `run_square`/`run_rect` replace load() with one/two
files (src/lib.rs:367-474), `run_stream_batch` replaces stream()'s inner loops
(src/lib.rs:322-333).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import (ALLGATHER_FN, GROUP_NONE, LD_SINK, LINKS_CHUNK, LINKS_SINK, LINKS_TALLIES, LINKS_VALUES, SLAB_SINK,
                   STREAM_GROUPS_LOADED, STREAM_GROUPS_STREAMED, STREAM_SUMMARY_LOADED, STREAM_SUMMARY_STREAMED, DistanceError,
                   GroupCell, LaunchInfo, LdBin, PairsInfo, SITE_CLASSES, SiteWindow, SummaryTotals, load)

MEASURES = {"n": 0, "n_high": 1, "raw": 2, "jc69": 3, "k80": 4, "tn93": 5}
INT_MEASURES = ("n", "n_high")
FLOAT_MEASURES = ("raw", "jc69", "k80", "tn93")
OUT_DISTANCE, OUT_TALLY, OUT_TALLY16 = 0, 1, 2
FIN_CLOSE = 0x100
PATHS = {"auto": 0, "dense": 1, "consensus": 2, "hybrid": 3}
MATRIX_STYLES = {"tsv": 0, "phylip": 1}


def _measure_id(measure) -> int:
    if isinstance(measure, str):
        m = load().dst_measure_from_name(measure.encode())
        if m < 0:
            raise ValueError(f"Unknown distance measure {measure!r}")  # src/lib.rs:486
        return m
    return int(measure)


def tally_width(measure) -> int:
    return load().dst_tally_width(_measure_id(measure))


def square_pairs(n: int) -> int:
    return int(load().dst_square_pairs(n))


def square_row_start(n: int, i: int) -> int:
    return int(load().dst_square_row_start(n, i))


def partition_square(n: int, parts: int) -> list[int]:
    """Row bounds of `parts` contiguous row ranges with near-equal pair counts (multi-GPU cut)."""
    b = (C.c_uint64 * (parts + 1))()
    rc = load().dst_partition_square(n, parts, b)
    if rc:
        raise DistanceError(rc, "dst_partition_square")
    return [int(x) for x in b]


def partition_rect(n_rows: int, parts: int) -> list[int]:
    b = (C.c_uint64 * (parts + 1))()
    rc = load().dst_partition_rect(n_rows, parts, b)
    if rc:
        raise DistanceError(rc, "dst_partition_rect")
    return [int(x) for x in b]


def sliding_windows(length: int, width: int, step: int) -> np.ndarray:
    """The (k, 2) windows [begin, end) of `--windows width --step step` over `length` columns (dst_sliding_windows)."""
    count = C.c_uint32()
    rc = load().dst_sliding_windows(length, width, step, None, None, 0, C.byref(count))
    if rc:
        raise DistanceError(rc, f"dst_sliding_windows: {int(count.value)} windows")
    k = int(count.value)
    begin, end = np.zeros(max(k, 1), np.uint64), np.zeros(max(k, 1), np.uint64)
    rc = load().dst_sliding_windows(length, width, step, begin.ctypes.data, end.ctypes.data, k, C.byref(count))
    if rc:
        raise DistanceError(rc, "dst_sliding_windows")
    return np.stack([begin[:k], end[:k]], axis=1)


def site_stats(counts, windows, group_sizes, site_begin: int = 0) -> dict:
    """Engine.site_counts' (sites, G, 5) entries of the sites from `site_begin` reduced to windows (dst_site_stats, pure
    host code): a dict of (n_windows, G) arrays `records`, `sites`, `called`, `segregating` (uint64), `theta_sum` and
    `pi_sum` (float64).  Watterson's theta per site is theta_sum / called, the per-site pi is pi_sum / called."""
    c = np.ascontiguousarray(counts, np.uint32)
    if c.ndim != 3 or c.shape[2] != SITE_CLASSES or c.shape[1] == 0:
        raise ValueError(f"counts must be a (sites, groups, {SITE_CLASSES}) array")
    sites, G = int(c.shape[0]), int(c.shape[1])
    sizes = np.ascontiguousarray(group_sizes, np.uint64)
    if sizes.shape != (G,):
        raise ValueError(f"group_sizes must hold one size per group ({G})")
    begin, end, nw = _window_arrays(windows)
    out = (SiteWindow * max(nw * G, 1))()
    anchor = c if c.size else np.zeros(1, np.uint32)   # (never a NULL array)
    rc = load().dst_site_stats(anchor.ctypes.data, site_begin, site_begin + sites, G, begin.ctypes.data, end.ctypes.data, nw,
                               sizes.ctypes.data, C.addressof(out), nw * G)
    if rc:
        raise DistanceError(rc, "dst_site_stats: a window outside the counted sites" if rc == 1 else "dst_site_stats")
    rec = np.frombuffer(out, dtype=np.dtype([("records", "<u8"), ("sites", "<u8"), ("called", "<u8"), ("segregating", "<u8"),
                                             ("theta_sum", "<f8"), ("pi_sum", "<f8")]))[:nw * G].reshape(nw, G)
    return {name: rec[name].copy() for name in rec.dtype.names}


def site_major(counts, g: int = 0):
    """(allele uint8[sites], major uint32[sites], other uint32[sites]) of group `g` of Engine.site_counts' (sites, G, 5)
    entries (dst_site_major, pure host code): per site the class (0 A, 1 T, 2 G, 3 C) with the largest of the four base
    counts, ties to the smallest class, that count, and the sum of the other three."""
    c = np.ascontiguousarray(counts, np.uint32)
    if c.ndim != 3 or c.shape[2] != SITE_CLASSES or c.shape[1] == 0:
        raise ValueError(f"counts must be a (sites, groups, {SITE_CLASSES}) array")
    sites, G = int(c.shape[0]), int(c.shape[1])
    allele, major, other = np.zeros(max(sites, 1), np.uint8), np.zeros(max(sites, 1), np.uint32), np.zeros(max(sites, 1), np.uint32)
    anchor = c if c.size else np.zeros(1, np.uint32)
    rc = load().dst_site_major(anchor.ctypes.data, sites, G, int(g), allele.ctypes.data, major.ctypes.data, other.ctypes.data)
    if rc:
        raise DistanceError(rc, "dst_site_major: g is not a group of the counts")
    return allele[:sites], major[:sites], other[:sites]


def ld_finalize(tallies) -> dict:
    """{"r2", "d", "dprime"}: float64 arrays, one entry per row {m, a, b, c} of `tallies` (dst_ld_finalize, pure host code,
    every operation fixed by the header); NaN where the statistic is not defined."""
    t = np.ascontiguousarray(tallies, np.uint32)
    if t.ndim != 2 or t.shape[1] != 4:
        raise ValueError("tallies must be an (n_pairs, 4) array")
    n = int(t.shape[0])
    out = {k: np.zeros(max(n, 1), np.float64) for k in ("r2", "d", "dprime")}
    anchor = t if n else np.zeros(4, np.uint32)
    rc = load().dst_ld_finalize(anchor.ctypes.data, n, out["r2"].ctypes.data, out["d"].ctypes.data, out["dprime"].ctypes.data)
    if rc:
        raise DistanceError(rc, "dst_ld_finalize")
    return {k: v[:n] for k, v in out.items()}


def ld_band(sites, max_gap: int):
    """(row_end uint32[S], pairs, tiles) of the band of `max_gap` over the strictly ascending `sites` (dst_ld_band, pure host
    code): the band pairs of position p are p < q < row_end[p]; `pairs` their number; `tiles` the 64 x 64 position tiles
    that hold one, which is what the band kernels launch."""
    s = np.ascontiguousarray(sites, np.uint32).ravel()
    S = len(s)
    row_end = np.zeros(max(S, 1), np.uint32)
    pairs, tiles = C.c_uint64(), C.c_uint64()
    anchor = s if S else np.zeros(1, np.uint32)
    rc = load().dst_ld_band(anchor.ctypes.data, S, int(max_gap), row_end.ctypes.data, C.byref(pairs), C.byref(tiles))
    if rc:
        raise DistanceError(rc, "dst_ld_band: the list must be strictly ascending")
    return row_end[:S], int(pairs.value), int(tiles.value)


def _window_arrays(windows):
    w = np.asarray(windows)
    if w.size == 0:
        w = np.zeros((0, 2), np.uint64)
    if w.ndim != 2 or w.shape[1] != 2:
        raise ValueError("windows must be an (n_windows, 2) array of [begin, end)")
    if w.dtype.kind not in "iu":
        raise ValueError("windows must be integers")
    if w.dtype.kind == "i" and w.size and int(w.min()) < 0:
        raise ValueError("windows must not be negative")
    begin = np.ascontiguousarray(w[:, 0], np.uint64)
    end = np.ascontiguousarray(w[:, 1], np.uint64)
    if begin.size == 0:   # (never a NULL array, also for an empty list)
        return np.zeros(1, np.uint64), np.zeros(1, np.uint64), 0
    return begin, end, int(begin.size)


def shared_range(n: int, rank: int, world: int) -> tuple[int, int]:
    """The records rank `rank` of `world` packs and lists in a shared upload (dst_shared_range)."""
    b, e = C.c_uint64(), C.c_uint64()
    rc = load().dst_shared_range(n, rank, world, C.byref(b), C.byref(e))
    if rc:
        raise DistanceError(rc, "dst_shared_range")
    return int(b.value), int(e.value)


def plan_tiles(square: bool, row_begin: int, row_end: int, n_cols: int, measure, variant: int = 0):
    """Tile schedule of one launch: (tiles[(i0, j0)...] with idle fillers dropped, tile_rows, tile_cols)."""
    m = _measure_id(measure)
    count, bm, bn = C.c_size_t(), C.c_int(), C.c_int()
    lib = load()
    rc = lib.dst_plan_tiles(int(square), row_begin, row_end, n_cols, m, variant, None, 0, C.byref(count),
                            C.byref(bm), C.byref(bn))
    if rc:
        raise DistanceError(rc, "dst_plan_tiles")
    ij = np.zeros((max(count.value, 1), 2), np.uint32)
    rc = lib.dst_plan_tiles(int(square), row_begin, row_end, n_cols, m, variant, ij.ctypes.data,
                            count.value, C.byref(count), None, None)
    if rc:
        raise DistanceError(rc, "dst_plan_tiles")
    ij = ij[:count.value]
    return ij, bm.value, bn.value


_PATH_NAMES = {1: "dense", 2: "consensus", 3: "hybrid"}
_MEASURE_NAMES = {v: k for k, v in MEASURES.items()}


def _launch_dict(li: LaunchInfo) -> dict:
    d = {name: getattr(li, name) for name, _ in LaunchInfo._fields_}
    d["path"] = _PATH_NAMES.get(li.path)
    d["measure"] = _MEASURE_NAMES.get(li.measure)
    for key in ("wide", "square", "hot", "run_records"):
        d[key] = bool(d[key])
    return d


def plan_consensus_launch(measure, out_kind: int = OUT_DISTANCE, wide: bool = False, square: bool = True, n_rows: int = 0,
                          n_cols: int = 0, total_pairs: int | None = None, events_per_pair: float = 0.0,
                          list_length: float = 0.0, run_adds: float = 0.0, hot: bool = False) -> dict:
    """Which consensus pair kernel variant and tile height a launch of n_rows rows against n_cols column records would get
    (dst_plan_consensus_launch; no GPU needed): a dict like Engine.last_launch()."""
    if total_pairs is None:
        total_pairs = n_rows * n_cols
        if square:   # rows [0, n_rows) of the n_cols x n_cols triangle
            total_pairs = n_rows * n_cols - n_rows * (n_rows + 1) // 2
    li = LaunchInfo()
    rc = load().dst_plan_consensus_launch(_measure_id(measure), int(out_kind), int(wide), int(square), int(n_rows), int(n_cols),
                                          int(total_pairs), float(events_per_pair), float(list_length), float(run_adds),
                                          int(hot), C.byref(li))
    if rc:
        raise DistanceError(rc, "dst_plan_consensus_launch")
    return _launch_dict(li)


def finalize(measure, tallies, q_counts=None, t_counts=None):
    """Host finalisation in the reference's f64 operation order (dst_finalize)."""
    m = _measure_id(measure)
    t = np.ascontiguousarray(tallies, np.uint32)
    qc = None if q_counts is None else np.ascontiguousarray(q_counts, np.uint32)
    tc = None if t_counts is None else np.ascontiguousarray(t_counts, np.uint32)
    f, i = C.c_double(), C.c_int64()
    rc = load().dst_finalize(m, t.ctypes.data, None if qc is None else qc.ctypes.data,
                             None if tc is None else tc.ctypes.data, C.byref(f), C.byref(i))
    if rc:
        raise DistanceError(rc, "dst_finalize")
    return int(i.value) if m in (0, 1) else float(f.value)


def format_distance(measure, value) -> str:
    m = _measure_id(measure)
    buf = C.create_string_buffer(64)
    if m in (0, 1):
        load().dst_format_distance(m, 0.0, int(value), buf, 64)
    else:
        load().dst_format_distance(m, float(value), 0, buf, 64)
    return buf.value.decode()


def newick(parent, length, ids, support=None) -> bytes:
    """Newick text of a tree from Engine.nj / nj_matrix (dst_newick): ids name the leaves 0..n-1 (str or bytes).
    support: uint32[2n-2] from Engine.nj_bootstrap, written after every internal non-root node's ')' (dst_newick_support);
    None gives dst_newick's text."""
    parent = np.ascontiguousarray(parent, np.uint32)
    length = np.ascontiguousarray(length, np.float64)
    names = [i.encode() if isinstance(i, str) else bytes(i) for i in ids]
    n = len(names)
    chars = b"".join(names)
    offsets = np.zeros(n + 1, np.uint64)
    offsets[1:] = np.cumsum([len(x) for x in names], dtype=np.uint64) if n else []
    if len(parent) != max(2 * n - 2, 0) or len(length) != len(parent):
        raise ValueError("parent and length need 2n - 2 entries for n ids")
    lib = load()
    if support is None:
        name = "dst_newick"
        call = lambda out, cap, need: lib.dst_newick(n, parent.ctypes.data, length.ctypes.data, chars,  # noqa: E731
                                                     offsets.ctypes.data, out, cap, need)
    else:
        support = np.ascontiguousarray(support, np.uint32)
        if len(support) != len(parent):
            raise ValueError("support needs 2n - 2 entries for n ids")
        name = "dst_newick_support"
        call = lambda out, cap, need: lib.dst_newick_support(n, parent.ctypes.data, length.ctypes.data,  # noqa: E731
                                                             chars, offsets.ctypes.data, support.ctypes.data, out,
                                                             cap, need)
    need = C.c_size_t(0)
    rc = call(None, 0, C.byref(need))
    if rc not in (0, 6):
        raise DistanceError(rc, f"{name}: malformed tree or arguments")
    buf = C.create_string_buffer(max(need.value, 1))
    rc = call(buf, need.value, C.byref(need))
    if rc:
        raise DistanceError(rc, name)
    return buf.raw[:need.value]


LINKAGES = ("average", "weighted", "complete")


def _linkage_id(linkage) -> int:
    if isinstance(linkage, str):
        if linkage not in LINKAGES:
            raise ValueError(f"unknown linkage {linkage!r}: one of {', '.join(LINKAGES)}")
        return LINKAGES.index(linkage)
    return int(linkage)


def newick_rooted(parent, length, ids) -> bytes:
    """Newick text of a tree from Engine.dendrogram / dendrogram_matrix (dst_newick_rooted): 2n - 1 nodes, a binary
    root; ids name the leaves 0..n-1 (str or bytes)."""
    parent = np.ascontiguousarray(parent, np.uint32)
    length = np.ascontiguousarray(length, np.float64)
    names = [i.encode() if isinstance(i, str) else bytes(i) for i in ids]
    n = len(names)
    chars = b"".join(names)
    offsets = np.zeros(n + 1, np.uint64)
    offsets[1:] = np.cumsum([len(x) for x in names], dtype=np.uint64) if n else []
    if len(parent) != max(2 * n - 1, 0) or len(length) != len(parent):
        raise ValueError("parent and length need 2n - 1 entries for n ids")
    lib = load()
    need = C.c_size_t(0)
    rc = lib.dst_newick_rooted(n, parent.ctypes.data, length.ctypes.data, chars, offsets.ctypes.data, None, 0,
                               C.byref(need))
    if rc not in (0, 6):
        raise DistanceError(rc, "dst_newick_rooted: malformed tree or arguments")
    buf = C.create_string_buffer(max(need.value, 1))
    rc = lib.dst_newick_rooted(n, parent.ctypes.data, length.ctypes.data, chars, offsets.ctypes.data, buf, need.value,
                               C.byref(need))
    if rc:
        raise DistanceError(rc, "dst_newick_rooted")
    return buf.raw[:need.value]


def bootstrap_columns(seed: int, replicate: int, length: int) -> np.ndarray:
    """The source column of every column of bootstrap replicate `replicate` (dst_bootstrap_columns): uint32[length]."""
    cols = np.zeros(max(int(length), 1), np.uint32)
    load().dst_bootstrap_columns(int(seed), int(replicate), int(length), cols.ctypes.data)
    return cols[:int(length)]


class Engine:
    """One GPU's context.  `device` is the HIP device ordinal."""

    def __init__(self, device: int = 0):
        self._lib = load()
        h = C.c_void_p()
        rc = self._lib.dst_create(device, C.byref(h))
        if rc:
            raise DistanceError(rc, self._lib.dst_last_error(None).decode())
        self._h = h
        self.device = device
        self.last_links_calls, self.last_links_first = [], []   # Engine.links: n_links / first_link of every sink call

    # ---- lifetime --------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.dst_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc: int):
        if rc:
            raise DistanceError(rc, self._lib.dst_last_error(self._h).decode())

    # ---- knobs -----------------------------------------------------------------------------
    def set_variant(self, variant: int):
        self._check(self._lib.dst_set_variant(self._h, variant))

    def set_ksplit(self, ksplit: int):
        """0 = automatic split over L for launches with few tiles, 1 = off, k = force."""
        self._check(self._lib.dst_set_ksplit(self._h, ksplit))

    def set_path(self, path):
        """"auto" (default), "dense" (bit-plane tiles, work ~ L) or "consensus" (difference lists against a
        per-site plurality sequence: the idea of the reference's -m n, src/measures.rs:28-53, for every measure)."""
        self._check(self._lib.dst_set_path(self._h, PATHS[path] if isinstance(path, str) else int(path)))

    def last_path(self) -> str:
        return {1: "dense", 2: "consensus", 3: "hybrid"}.get(self._lib.dst_last_path(self._h), "?")

    def last_launch(self) -> dict:
        """Which kernel variant the most recent pair launch was (dst_last_launch): path, measure, family, out_kind, wide,
        square, event_waves (EW of the consensus pair kernel as instantiated; 0: dense), heavy_events, rows_per_tile, tiles,
        hot, run_records, variant and ksplit (dense), pairs, and the sampled figures the choice was made from.
        path is None before the first launch."""
        li = LaunchInfo()
        self._check(self._lib.dst_last_launch(self._h, C.byref(li)))
        return _launch_dict(li)

    def run_records(self, slot: int = 0) -> tuple[int, int]:
        """(records the consensus path treats as run records — long runs of N left out of their lists —, entries removed)"""
        a, b = C.c_uint64(), C.c_uint64()
        self._check(self._lib.dst_run_records(self._h, slot, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def planes_stored(self, slot: int = 0) -> bool:
        """False while the upload has deferred the set's bit-planes (a set prepared for the consensus path: dst_planes_stored)"""
        v = C.c_int()
        self._check(self._lib.dst_planes_stored(self._h, slot, C.byref(v)))
        return bool(v.value)

    # ---- per-alignment precompute of -m n (src/lib.rs:223-231) ------------------------------
    def consensus(self, both_slots: bool = False) -> np.ndarray:
        """consensus() of src/fastaio.rs:289-336 over slot 0 (and slot 1), computed on the device."""
        _, length = self.set_info(0)
        out = np.zeros(length, np.uint8)
        self._check(self._lib.dst_consensus(self._h, int(both_slots), out.ctypes.data, out.nbytes))
        return out

    def differences(self, slot: int, other: np.ndarray) -> list[np.ndarray]:
        """get_differences() of src/fastaio.rs:67-75 for every record of `slot` against `other`."""
        n, _ = self.set_info(slot)
        other = np.ascontiguousarray(other, np.uint8)
        offsets = np.zeros(n + 1, np.uint64)
        total = C.c_uint64()
        self._check(self._lib.dst_differences(self._h, slot, other.ctypes.data, other.size, offsets.ctypes.data,
                                              None, 0, C.byref(total)))
        sites = np.zeros(max(total.value, 1), np.uint32)
        self._check(self._lib.dst_differences(self._h, slot, other.ctypes.data, other.size, offsets.ctypes.data,
                                              sites.ctypes.data, sites.size, C.byref(total)))
        return [sites[int(offsets[r]):int(offsets[r + 1])] for r in range(n)]

    # ---- input -----------------------------------------------------------------------------
    def upload(self, slot: int, codes: np.ndarray, base_counts: np.ndarray | None = None):
        """codes: (n, L) uint8 Paradis codes (any row stride); base_counts: (n, 4) {A,T,G,C}."""
        codes = np.asarray(codes)
        if codes.dtype != np.uint8 or codes.ndim != 2:
            raise ValueError("codes must be a 2-D uint8 array")
        # rows must run forwards in memory, at least one row apart (a reversed view has a negative stride)
        if codes.shape[1] and (codes.strides[1] != 1 or (codes.shape[0] > 1 and codes.strides[0] < codes.shape[1])):
            codes = np.ascontiguousarray(codes)
        stride = codes.strides[0] if codes.shape[0] > 1 else max(codes.shape[1], 1)
        bc = None
        if base_counts is not None:
            bc = np.ascontiguousarray(base_counts, np.uint32)
            if bc.shape != (codes.shape[0], 4):
                raise ValueError("base_counts must be (n, 4)")
        self._check(self._lib.dst_upload(self._h, slot, codes.ctypes.data, codes.shape[0], codes.shape[1],
                                         stride, None if bc is None else bc.ctypes.data))

    def upload_device(self, slot: int, d_ptr: int, n: int, length: int, row_stride: int,
                      d_counts_ptr: int | None = None, stream: int | None = None):
        self._check(self._lib.dst_upload_device(self._h, slot, d_ptr, n, length, row_stride, d_counts_ptr,
                                                stream))

    def upload_shared(self, comm: "Comm", slot: int, d_ptr: int, n: int, length: int, row_stride: int,
                      with_counts: bool = False, stream: int | None = None):
        """Collective: this rank packs and lists its share of the records, one all-gather brings everybody's lists
        (dst_upload_shared)."""
        self._check(self._lib.dst_upload_shared(comm._h, slot, d_ptr, n, length, row_stride, int(with_counts), stream))

    def shared_stats(self, slot: int = 0) -> dict:
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self._lib.dst_shared_stats(self._h, slot, C.byref(a), C.byref(b), C.byref(c)))
        return {"shared_uploads": int(a.value), "fallbacks": int(b.value), "block_entries": int(c.value)}

    def set_info(self, slot: int) -> tuple[int, int]:
        n, length = C.c_size_t(), C.c_size_t()
        self._check(self._lib.dst_set_info(self._h, slot, C.byref(n), C.byref(length)))
        return int(n.value), int(length.value)

    def base_counts(self, slot: int) -> np.ndarray:
        n, _ = self.set_info(slot)
        out = np.zeros((n, 4), np.uint32)
        self._check(self._lib.dst_get_base_counts(self._h, slot, out.ctypes.data))
        return out

    # ---- runs into host memory ---------------------------------------------------------------
    def _alloc(self, m: int, out_kind: int, pairs: int) -> np.ndarray:
        if out_kind == OUT_TALLY:
            return np.zeros((pairs, self._lib.dst_tally_width(m)), np.uint32)
        if out_kind == OUT_TALLY16:
            return np.zeros((pairs, self._lib.dst_tally_width(m)), np.uint16)
        return np.zeros(pairs, np.int64 if m in (0, 1) else np.float64)

    def run_square(self, measure, row_begin: int = 0, row_end: int | None = None,
                   tallies: bool = False, tallies16: bool = False) -> np.ndarray:
        """Distances (or tallies) of pairs (i, j), row_begin <= i < row_end, j > i, canonical order."""
        m = _measure_id(measure)
        n, _ = self.set_info(0)
        row_end = n if row_end is None else row_end
        pairs = square_row_start(n, min(row_end, n)) - square_row_start(n, min(row_begin, n)) \
            if row_end > row_begin else 0
        kind = OUT_TALLY16 if tallies16 else OUT_TALLY if tallies else OUT_DISTANCE
        out = self._alloc(m, kind, pairs)
        self._check(self._lib.dst_run_square_host(self._h, m, row_begin, row_end, kind, out.ctypes.data,
                                                  out.nbytes))
        return out

    def run_rect(self, measure, row_slot: int = 0, col_slot: int = 1, row_begin: int = 0,
                 row_end: int | None = None, tallies: bool = False, tallies16: bool = False) -> np.ndarray:
        """Distances (or tallies) of rows [row_begin, row_end) of row_slot against every record of col_slot:
        [row - row_begin][column]."""
        m = _measure_id(measure)
        n_rows, _ = self.set_info(row_slot)
        n_cols, _ = self.set_info(col_slot)
        row_end = n_rows if row_end is None else row_end
        kind = OUT_TALLY16 if tallies16 else OUT_TALLY if tallies else OUT_DISTANCE
        out = self._alloc(m, kind, max(row_end - row_begin, 0) * n_cols)
        self._check(self._lib.dst_run_rect_host(self._h, m, row_slot, col_slot, row_begin, row_end, kind,
                                                out.ctypes.data, out.nbytes))
        return out.reshape((max(row_end - row_begin, 0), n_cols) + out.shape[1:])

    def run_stream_batch(self, measure, batch_codes: np.ndarray, batch_counts=None,
                         tallies: bool = False) -> np.ndarray:
        """One streamed batch against the loaded set in slot 0 (src/lib.rs:322-333): returns
        [streamed record][loaded record], i.e. the reference's streamed-major output order."""
        self.upload(1, batch_codes, batch_counts)
        return self.run_rect(measure, row_slot=1, col_slot=0, tallies=tallies)

    def stream(self, measure, max_records: int, depth: int = 3, tallies: bool = False, nibbles: bool = False) -> "Stream":
        """The overlapped stream-mode pipeline (dst_stream_*): batches against the loaded set of slot 0.
        nibbles: the 4-bit wire format (DST_WIRE_NIBBLES): push() packs the codes' high nibbles, two sites per byte."""
        return Stream(self, measure, max_records, depth, tallies, nibbles)

    def closest_stream(self, measure, k: int, max_records: int, side: str = "loaded", depth: int = 3,
                       nibbles: bool = False) -> "ClosestStream":
        """A stream that keeps the k nearest records instead of the result matrix (dst_stream_open_closest).
        side="loaded": every loaded record's k nearest streamed records over the whole stream (result());
        side="streamed": every streamed record's k nearest loaded records, per batch (pop())."""
        return ClosestStream(self, measure, k, max_records, side, depth, nibbles)

    def window_closest_stream(self, measure, windows, k: int, max_records: int, depth: int = 3, nibbles: bool = False,
                              max_entries: int = 0) -> "WindowClosestStream":
        """A stream that keeps, for every (loaded record, column window), the k nearest streamed records
        (dst_stream_open_window_closest): nearest_windows() against a panel that does not fit on the GPU.
        max_entries: the most tallies of one device range (0: the default); the result does not depend on it."""
        return WindowClosestStream(self, measure, windows, k, max_records, depth, nibbles, max_entries)

    def links_stream(self, measure, threshold: float, max_records: int, depth: int = 3, nibbles: bool = False,
                     values: bool = True, tallies: bool = False, window: int = 0) -> "LinksStream":
        """A stream that hands back the pairs within `threshold` instead of the result matrix (dst_stream_open_links):
        per batch (n_records, streamed, loaded[, values][, tallies]), by dst_links' rule, in the stream's own order.
        window: the most links of one window (0: the default); the result does not depend on it."""
        return LinksStream(self, measure, threshold, max_records, depth, nibbles, values, tallies, window)

    def summary_stream(self, measure, max_records: int, threshold: float = 0.0, loaded: bool = True, streamed: bool = False,
                       bins: int = 0, width: float = 1.0, depth: int = 3, nibbles: bool = False) -> "SummaryStream":
        """A stream that keeps summary()'s counts and exact sums instead of the result matrix (dst_stream_open_summary).
        loaded: every loaded record's `within`, `summable` and `sum` over the whole stream (result()); streamed: the same
        for every streamed record over the loaded set, per batch (pop()); bins: the histogram of every pair so far."""
        return SummaryStream(self, measure, max_records, threshold, loaded, streamed, bins, width, depth, nibbles)

    def group_summary_stream(self, measure, max_records: int, loaded_groups=None, n_loaded_groups=None,
                             n_streamed_groups: int = 1, threshold: float = float("inf"), loaded: bool = False,
                             streamed: bool = False, depth: int = 3, nibbles: bool = False) -> "GroupSummaryStream":
        """A stream that keeps group_summary()'s cells of (every record so far) x (the loaded set) instead of the result
        matrix (dst_stream_open_group_summary).  loaded_groups: one label per loaded record as for group_summary() (None:
        all in group 0); the streamed records' labels come with every push().  streamed: every batch's records' table over
        the loaded groups (pop()); loaded: every loaded record's table over the streamed groups (result())."""
        return GroupSummaryStream(self, measure, max_records, loaded_groups, n_loaded_groups, n_streamed_groups, threshold,
                                  loaded, streamed, depth, nibbles)

    def run_slabs(self, measure, sink, max_pairs: int, square: bool = True, row_slot: int = 0, col_slot: int = 1,
                  tallies: bool = False):
        """In-order slab sink (dst_run_slabs): sink(first_pair, rb, re, array) per slab; a truthy return stops."""
        m = _measure_id(measure)
        kind = OUT_TALLY if tallies else OUT_DISTANCE
        width = self._lib.dst_tally_width(m)

        def _cb(_user, first, n_pairs, rb, re, data):
            if tallies:
                arr = np.ctypeslib.as_array(C.cast(data, C.POINTER(C.c_uint32)), shape=(n_pairs, width))
            elif m in (0, 1):
                arr = np.ctypeslib.as_array(C.cast(data, C.POINTER(C.c_int64)), shape=(n_pairs,))
            else:
                arr = np.ctypeslib.as_array(C.cast(data, C.POINTER(C.c_double)), shape=(n_pairs,))
            return 1 if sink(int(first), int(rb), int(re), arr) else 0

        cb = SLAB_SINK(_cb)
        self._check(self._lib.dst_run_slabs(self._h, m, int(square), row_slot, col_slot, kind, max_pairs, cb, None))

    def nearest(self, measure, k: int, square: bool = True, row_slot: int = 0, col_slot: int = 1, tallies: bool = False):
        """The k nearest records of every row record (dst_nearest): (index[n_rows, k_used], values[n_rows, k_used]), plus
        tallies[n_rows, k_used, width] when asked.  Ascending by (key of the value, index); square: slot 0 against itself
        without the diagonal, the canonical pair's value; else row_slot against every record of col_slot."""
        m = _measure_id(measure)
        n_rows, _ = self.set_info(0 if square else row_slot)
        n_cols, _ = self.set_info(0 if square else col_slot)
        ku = min(int(k), max(n_rows - 1, 0) if square else n_cols) if 1 <= int(k) <= 256 else 0
        width = self._lib.dst_tally_width(m)
        index = np.zeros((n_rows, ku), np.uint32)
        values = np.zeros((n_rows, ku), np.int64 if m in (0, 1) else np.float64)
        tal = np.zeros((n_rows, ku, width), np.uint32) if tallies else None
        k_used = C.c_uint32()
        self._check(self._lib.dst_nearest(self._h, m, int(square), row_slot, col_slot, int(k), index.ctypes.data,
                                          None if tal is None else tal.ctypes.data, values.ctypes.data, n_rows * ku,
                                          C.byref(k_used)))
        assert k_used.value == ku
        return (index, values, tal) if tallies else (index, values)

    def clusters(self, measure, threshold: float, max_pairs: int = 0):
        """Single-linkage clusters of slot 0 (dst_clusters): (labels uint32[n], links).  Records i < j are linked when the
        pair's DST_OUT_DISTANCE payload v <= threshold (int measures: v <= floor(threshold); NaN never links);
        labels[i] = the smallest record of i's cluster, links = the number of linked pairs.  max_pairs: the most pairs
        of one row slab (0: the default)."""
        m = _measure_id(measure)
        n, _ = self.set_info(0)
        labels = np.zeros(max(n, 1), np.uint32)   # (never a NULL label, also for an empty set)
        n_clusters, links = C.c_uint64(), C.c_uint64()
        self._check(self._lib.dst_clusters(self._h, m, float(threshold), int(max_pairs), labels.ctypes.data, n,
                                           C.byref(n_clusters), C.byref(links)))
        return labels[:n], int(links.value)

    def representatives(self, measure, threshold: float, max_pairs: int = 0, values: bool = True, tallies: bool = False):
        """Greedy representatives of slot 0 (dst_representatives): (rep uint32[n], values[n][, tallies[n, width]]).  In input
        order a record is a representative unless an earlier representative is linked to it (dst_clusters' rule against
        `threshold`); rep[j] = j then, otherwise the smallest representative linked to j.  values (int64 for n / n_high,
        float64 otherwise) and tallies (uint32) are those of the pair (rep[j], j), bitwise run_square's, and all-zero bits for a
        representative.  max_pairs: the most pairs of one row slab (0: the default); the result does not depend on it.
        last_representatives keeps the number of representatives."""
        m = _measure_id(measure)
        n, _ = self.set_info(0)
        width = self._lib.dst_tally_width(m)
        rep = np.zeros(max(n, 1), np.uint32)   # (never a NULL rep, also for an empty set)
        val = np.zeros(max(n, 1), np.int64 if m in (0, 1) else np.float64) if values else None
        tal = np.zeros((max(n, 1), width), np.uint32) if tallies else None
        count = C.c_uint64()
        self._check(self._lib.dst_representatives(self._h, m, float(threshold), int(max_pairs), rep.ctypes.data,
                                                  None if tal is None else tal.ctypes.data,
                                                  None if val is None else val.ctypes.data, n, C.byref(count)))
        self.last_representatives = int(count.value)
        out = (rep[:n],)
        if values:
            out += (val[:n],)
        if tallies:
            out += (tal[:n],)
        return out

    def links(self, measure, threshold: float, square: bool = True, row_slot: int = 0, col_slot: int = 1, max_pairs: int = 0,
              values: bool = True, tallies: bool = False, count_only: bool = False):
        """The pairs within `threshold` (dst_links), in canonical pair order: (row uint32[n_links], col uint32[n_links]), then
        values[n_links] (int64 / float64, bitwise run_square's / run_rect's) and tallies[n_links, width] (uint32) when asked.
        A pair is a link by dst_clusters' rule (int measures: v <= floor(threshold); f64: IEEE v <= threshold, NaN never).
        square: slot 0, pairs row < col; else every record of row_slot against every record of col_slot.  count_only: the
        int n_links, nothing copied.  The arrays are copied out of the library's buffers during the sink's calls;
        last_links_calls keeps the n_links of every call, last_links_first its first_link.  max_pairs: the most pairs of one row slab (0: the default); the
        result does not depend on it."""
        m = _measure_id(measure)
        width = self._lib.dst_tally_width(m)
        total = C.c_uint64()
        self.last_links_calls, self.last_links_first = [], []
        if count_only:
            self._check(self._lib.dst_links(self._h, m, int(square), row_slot, col_slot, float(threshold), int(max_pairs), 0,
                                            None, None, C.byref(total)))
            return int(total.value)
        vtype = np.int64 if m in (0, 1) else np.float64
        parts = ([], [], [], [])

        def _cb(_user, first, count, row, col, val, tal):
            count = int(count)
            self.last_links_calls.append(count)
            self.last_links_first.append(int(first))
            parts[0].append(np.ctypeslib.as_array(C.cast(row, C.POINTER(C.c_uint32)), shape=(count,)).copy())
            parts[1].append(np.ctypeslib.as_array(C.cast(col, C.POINTER(C.c_uint32)), shape=(count,)).copy())
            if values:
                parts[2].append(np.ctypeslib.as_array(C.cast(val, C.POINTER(C.c_int64)), shape=(count,)).view(vtype).copy())
            if tallies:
                parts[3].append(np.ctypeslib.as_array(C.cast(tal, C.POINTER(C.c_uint32)), shape=(count, width)).copy())
            return 0

        cb = LINKS_SINK(_cb)
        what = (LINKS_VALUES if values else 0) | (LINKS_TALLIES if tallies else 0)
        self._check(self._lib.dst_links(self._h, m, int(square), row_slot, col_slot, float(threshold), int(max_pairs), what,
                                        cb, None, C.byref(total)))
        assert int(total.value) == sum(self.last_links_calls)

        def cat(p, dtype, shape):
            return np.concatenate(p) if p else np.zeros(shape, dtype)

        out = (cat(parts[0], np.uint32, 0), cat(parts[1], np.uint32, 0))
        if values:
            out += (cat(parts[2], vtype, 0),)
        if tallies:
            out += (cat(parts[3], np.uint32, (0, width)),)
        return out

    def pair_sites(self, measure, row, col, square: bool = True, row_slot: int = 0, col_slot: int = 1, count_only: bool = False):
        """The difference sites of the listed pairs (dst_pair_sites), CSR: (offsets uint64[n_pairs + 1], sites uint32[total],
        bases uint8[total]), or offsets alone with count_only.  Pair e is record row[e] against record col[e] (square: both
        of slot 0, any order, repeats and row == col allowed; else of row_slot and col_slot); its entries
        [offsets[e], offsets[e + 1]) are the ascending 0-based sites that add 1 to the measure's difference tally, with
        bases = the row record's nibble << 4 | the column record's (A 8, G 4, C 2, T 1)."""
        m = _measure_id(measure)
        row = np.ascontiguousarray(row, np.uint32).ravel()
        col = np.ascontiguousarray(col, np.uint32).ravel()
        if row.size != col.size:
            raise ValueError("row and col must have the same length")
        n_pairs = int(row.size)
        rbuf = row if n_pairs else np.zeros(1, np.uint32)   # (never a NULL index array, also for an empty list)
        cbuf = col if n_pairs else np.zeros(1, np.uint32)
        offsets = np.zeros(n_pairs + 1, np.uint64)
        total = C.c_uint64()
        self._check(self._lib.dst_pair_sites(self._h, m, int(square), row_slot, col_slot, rbuf.ctypes.data, cbuf.ctypes.data,
                                             n_pairs, offsets.ctypes.data, None, None, 0, C.byref(total)))
        if count_only:
            return offsets
        cap = max(int(total.value), 1)
        sites, bases = np.zeros(cap, np.uint32), np.zeros(cap, np.uint8)
        self._check(self._lib.dst_pair_sites(self._h, m, int(square), row_slot, col_slot, rbuf.ctypes.data, cbuf.ctypes.data,
                                             n_pairs, offsets.ctypes.data, sites.ctypes.data, bases.ctypes.data, cap,
                                             C.byref(total)))
        return offsets, sites[:int(total.value)], bases[:int(total.value)]

    def run_pairs(self, measure, row, col, square: bool = True, row_slot: int = 0, col_slot: int = 1, values: bool = True,
                  tallies: bool = False, route: str = "auto", max_pairs: int = 0, info: bool = False):
        """The distances of the listed pairs and only these (dst_run_pairs): values (n_pairs,) int64 / f64 and/or tallies
        (n_pairs, width) uint32, bitwise what run_square / run_rect gives for each pair; plus the info dict when asked.
        Pair e is record row[e] against record col[e] (square: both of slot 0, any order, repeats and row == col allowed —
        (j, i) is the canonical pair (i, j), (i, i) the record against itself; else of row_slot and col_slot).  route:
        "auto", "direct" (from the two records' planes) or "sweep" (gathered from the row slabs of at most max_pairs pairs
        that the list touches; 0: the default); the result does not depend on either."""
        m = _measure_id(measure)
        routes = {"auto": 0, "direct": 1, "sweep": 2}
        r = routes.get(route, route)   # (anything else goes to the library as it is: its refusal)
        row = np.ascontiguousarray(row, np.uint32).ravel()
        col = np.ascontiguousarray(col, np.uint32).ravel()
        if row.size != col.size:
            raise ValueError("row and col must have the same length")
        n_pairs = int(row.size)
        rbuf = row if n_pairs else np.zeros(1, np.uint32)   # (never a NULL index array, also for an empty list)
        cbuf = col if n_pairs else np.zeros(1, np.uint32)
        width = self._lib.dst_tally_width(m)
        val = np.zeros(n_pairs, np.int64 if m in (0, 1) else np.float64) if values else None
        tal = np.zeros((n_pairs, width), np.uint32) if tallies else None
        pi = PairsInfo()
        # (an empty output array still has an address: NULL means "not wanted")
        vptr = (val.ctypes.data if n_pairs else rbuf.ctypes.data) if values else None
        tptr = (tal.ctypes.data if n_pairs else rbuf.ctypes.data) if tallies else None
        self._check(self._lib.dst_run_pairs(self._h, m, int(square), row_slot, col_slot, rbuf.ctypes.data, cbuf.ctypes.data,
                                            n_pairs, int(r), int(max_pairs), vptr, tptr, n_pairs, C.byref(pi)))
        out = ()
        if values:
            out += (val,)
        if tallies:
            out += (tal,)
        if info:
            out += ({"route": {1: "direct", 2: "sweep"}.get(pi.route, pi.route), "lanes_per_pair": int(pi.lanes_per_pair),
                     "direct_pairs": int(pi.direct_pairs), "swept_pairs": int(pi.swept_pairs), "slabs": int(pi.slabs)},)
        return out[0] if len(out) == 1 else out

    def run_windows(self, measure, windows, square: bool = True, row_slot: int = 0, col_slot: int = 1, row_begin: int = 0,
                    row_end: int | None = None, tallies: bool = False) -> np.ndarray:
        """Per column window [begin, end) of `windows` ((n_windows, 2) integers) what run_square / run_rect gives for rows
        [row_begin, row_end) on the sets cut to those columns (dst_run_windows): (n_windows, P) int64 / f64 in the
        canonical order of the range, or (n_windows, P, width) uint32 tallies."""
        m = _measure_id(measure)
        begin, end, nw = _window_arrays(windows)
        n_rows, _ = self.set_info(0 if square else row_slot)
        n_cols, _ = self.set_info(0 if square else col_slot)
        row_end = n_rows if row_end is None else row_end
        if row_end <= row_begin:
            pairs = 0
        elif square:
            pairs = square_row_start(n_cols, min(row_end, n_cols)) - square_row_start(n_cols, min(row_begin, n_cols))
        else:
            pairs = (row_end - row_begin) * n_cols
        kind = OUT_TALLY if tallies else OUT_DISTANCE
        out = self._alloc(m, kind, nw * pairs)
        self._check(self._lib.dst_run_windows_host(self._h, m, int(square), row_slot, col_slot, row_begin, row_end,
                                                   begin.ctypes.data, end.ctypes.data, nw, kind, out.ctypes.data, out.nbytes))
        return out.reshape((nw, pairs) + out.shape[1:])

    def window_base_counts(self, slot: int, windows) -> np.ndarray:
        """(n_windows, n, 4) {A,T,G,C} of every record of `slot`, counted by code inside every window."""
        begin, end, nw = _window_arrays(windows)
        n, _ = self.set_info(slot)
        out = np.zeros((nw, n, 4), np.uint32)
        self._check(self._lib.dst_window_base_counts(self._h, slot, begin.ctypes.data, end.ctypes.data, nw, out.ctypes.data,
                                                     out.size))
        return out

    def site_counts(self, slot: int = 0, groups=None, n_groups=None, begin: int = 0, end: int | None = None) -> np.ndarray:
        """(sites, G, 5) uint32: per site of [begin, end) and group the records whose code is exactly A, T, G, C, and those
        whose code names 2 or 3 bases (dst_site_counts).  `groups`: one integer label per record of `slot`, -1 or 2^32-1 for
        a record that belongs to no group (group_summary's rule); None: one group of every record.  n_groups defaults to
        the largest label + 1."""
        n, length = self.set_info(slot)
        if end is None:
            end = length
        if groups is None:
            labels, G = None, 1 if n_groups is None else int(n_groups)
        else:
            g = np.asarray(groups)
            if g.ndim != 1 or len(g) != n or not np.issubdtype(g.dtype, np.integer):
                raise ValueError(f"groups must be a 1-D integer array with one label per record ({n})")
            labels = _group_labels_u32(g, "groups")
            if n_groups is None:
                assigned = labels[labels != GROUP_NONE]
                n_groups = int(assigned.max()) + 1 if len(assigned) else 1
            G = int(n_groups)
            if len(labels) == 0:
                labels = np.zeros(1, np.uint32)   # (never a NULL array: NULL means one group)
        if not (0 <= begin <= GROUP_NONE * 2 ** 32 and 0 <= end <= GROUP_NONE * 2 ** 32 and 0 <= G <= GROUP_NONE):
            raise ValueError("begin, end and n_groups must be unsigned")
        sites = max(end - begin, 0)
        out = np.zeros((sites, G, SITE_CLASSES), np.uint32)
        anchor = out if out.size else np.zeros(1, np.uint32)
        self._check(self._lib.dst_site_counts(self._h, slot, None if labels is None else labels.ctypes.data, G, begin, end,
                                              anchor.ctypes.data, out.size))
        return out

    def _ld_inputs(self, sites, alleles, slot, groups, which):
        """the arrays of a site_ld call: (sites uint32, alleles uint8, labels uint32 or None); alleles None: the major
        allele of every listed site among the participating records (site_counts over the listed range + dst_site_major)"""
        n, _ = self.set_info(slot)
        s = np.ascontiguousarray(sites, np.uint32).ravel()
        labels = None
        if groups is not None:
            g = np.asarray(groups)
            if g.ndim != 1 or len(g) != n or not np.issubdtype(g.dtype, np.integer):
                raise ValueError(f"groups must be a 1-D integer array with one label per record ({n})")
            labels = _group_labels_u32(g, "groups")
            if len(labels) == 0:
                labels = np.zeros(1, np.uint32)   # (never a NULL array: NULL means every record)
        if alleles is None:
            a = np.zeros(len(s), np.uint8)
            if len(s):
                lo, hi = int(s.min()), int(s.max()) + 1
                member = None if labels is None else np.where(labels[:n] == np.uint32(which), 0, -1)
                counts = self.site_counts(slot, member, 1, lo, hi)
                a = site_major(counts, 0)[0][s.astype(np.int64) - lo]
        else:
            a = np.ascontiguousarray(alleles, np.uint8).ravel()
            if len(a) != len(s):
                raise ValueError("alleles must hold one allele per listed site")
        return s, np.ascontiguousarray(a, np.uint8), labels

    def site_ld(self, sites, alleles=None, slot: int = 0, groups=None, which: int = 0, row_begin: int = 0, row_end: int | None = None):
        """(tallies uint32[P, 4], alleles uint8[S]): {m, a, b, c} of the pairs of listed positions p < q with row_begin <= p
        < row_end, in canonical order (dst_site_ld).  `sites`: strictly ascending 0-based sites; `alleles`: the reference
        allele of each (0 A, 1 T, 2 G, 3 C), None: the major allele among the participating records.  `groups`: one integer
        label per record (-1: none); the records labelled `which` take part; None: every record."""
        s, a, labels = self._ld_inputs(sites, alleles, slot, groups, which)
        S = len(s)
        if row_end is None:
            row_end = S
        pairs = 0
        if 0 <= row_begin <= row_end <= S and S >= 2:
            pairs = square_row_start(S, min(row_end, S - 1)) - square_row_start(S, min(row_begin, S - 1))
        out = np.zeros((pairs, 4), np.uint32)
        anchor = out if pairs else np.zeros(4, np.uint32)
        sa, aa = (s, a) if S else (np.zeros(1, np.uint32), np.zeros(1, np.uint8))
        self._check(self._lib.dst_site_ld(self._h, slot, sa.ctypes.data, aa.ctypes.data, S, None if labels is None else labels.ctypes.data,
                                          which, row_begin, row_end, anchor.ctypes.data, pairs))
        return out, a

    def site_ld_band(self, sites, max_gap: int, alleles=None, slot: int = 0, groups=None, which: int = 0, row_begin: int = 0,
                     row_end: int | None = None):
        """(tallies uint32[P, 4], alleles uint8[S]): site_ld's {m, a, b, c} of the pairs with sites[q] - sites[p] <= max_gap
        and row_begin <= p < row_end, in canonical order (dst_site_ld_band); ld_band(sites, max_gap) names them."""
        s, a, labels = self._ld_inputs(sites, alleles, slot, groups, which)
        S = len(s)
        if row_end is None:
            row_end = S
        pairs = 0
        if 0 <= row_begin <= row_end <= S and S >= 2 and (np.diff(s.astype(np.int64)) > 0).all():
            ends = ld_band(s, max_gap)[0].astype(np.int64)
            pairs = int((ends - np.arange(S) - 1)[row_begin:row_end].sum())
        out = np.zeros((pairs, 4), np.uint32)
        anchor = out if pairs else np.zeros(4, np.uint32)
        sa, aa = (s, a) if S else (np.zeros(1, np.uint32), np.zeros(1, np.uint8))
        self._check(self._lib.dst_site_ld_band(self._h, slot, sa.ctypes.data, aa.ctypes.data, S, None if labels is None else labels.ctypes.data,
                                               which, int(max_gap), row_begin, row_end, anchor.ctypes.data, pairs))
        return out, a

    def site_ld_decay(self, sites, width: int, bins: int, min_r2: float = 0.0, alleles=None, slot: int = 0, groups=None, which: int = 0,
                      max_pairs: int = 0) -> dict:
        """The LD-decay curve (dst_site_ld_decay): {"pairs", "defined", "links" uint64[bins], "r2_sum" float64[bins], "alleles"}.
        Bin b holds the pairs with sites[q] - sites[p] in [b width, (b + 1) width); `defined` those with an r2, `links` those
        with r2 >= min_r2, r2_sum the exact fixed-point sum of r2 (units of 2^-LD_SCALE_BITS): the mean r2 is r2_sum / defined.
        max_pairs: the most band pairs one launch covers (0: the default); the result does not depend on it."""
        s, a, labels = self._ld_inputs(sites, alleles, slot, groups, which)
        S, B = len(s), int(bins)
        out = (LdBin * max(B, 1))()
        sa, aa = (s, a) if S else (np.zeros(1, np.uint32), np.zeros(1, np.uint8))
        self._check(self._lib.dst_site_ld_decay(self._h, slot, sa.ctypes.data, aa.ctypes.data, S, None if labels is None else labels.ctypes.data,
                                                which, float(min_r2), int(width), B, int(max_pairs), C.addressof(out), max(B, 0)))
        rows = np.frombuffer(out, np.dtype([("pairs", "<u8"), ("defined", "<u8"), ("links", "<u8"), ("r2_sum", "<f8")]))[:B]
        return {"pairs": rows["pairs"].copy(), "defined": rows["defined"].copy(), "links": rows["links"].copy(),
                "r2_sum": rows["r2_sum"].copy(), "alleles": a}

    def site_ld_links(self, sites, min_r2: float, alleles=None, slot: int = 0, groups=None, which: int = 0, max_pairs: int = 0,
                      count_only: bool = False, max_gap: int | None = None):
        """The pairs of listed positions whose r2 is defined and >= min_r2 (dst_site_ld_links), in canonical order:
        (pos_i uint32[L], pos_j uint32[L], tallies uint32[L, 4], alleles uint8[S]); count_only: the int L, nothing copied.
        The arguments are site_ld's; last_ld_calls keeps the n_links of every sink call, last_ld_first its first_link.
        max_pairs: the most site pairs of one row slab (0: the default); the result does not depend on it.  max_gap: only
        the links with sites[pos_j] - sites[pos_i] <= max_gap, from the band alone (dst_site_ld_links_band; max_pairs then counts
        band pairs); None: every link."""
        s, a, labels = self._ld_inputs(sites, alleles, slot, groups, which)
        S = len(s)
        sa, aa = (s, a) if S else (np.zeros(1, np.uint32), np.zeros(1, np.uint8))
        lp = None if labels is None else labels.ctypes.data
        total = C.c_uint64()
        self.last_ld_calls, self.last_ld_first = [], []

        def call(sink):
            head = (self._h, slot, sa.ctypes.data, aa.ctypes.data, S, lp, which, float(min_r2))
            tail = (int(max_pairs), sink, None, C.byref(total))
            if max_gap is None:
                return self._lib.dst_site_ld_links(*head, *tail)
            return self._lib.dst_site_ld_links_band(*head, int(max_gap), *tail)

        if count_only:
            self._check(call(None))
            return int(total.value)
        parts = ([], [], [])

        def _cb(_user, first, count, pos_i, pos_j, tal):
            count = int(count)
            self.last_ld_calls.append(count)
            self.last_ld_first.append(int(first))
            parts[0].append(np.ctypeslib.as_array(C.cast(pos_i, C.POINTER(C.c_uint32)), shape=(count,)).copy())
            parts[1].append(np.ctypeslib.as_array(C.cast(pos_j, C.POINTER(C.c_uint32)), shape=(count,)).copy())
            parts[2].append(np.ctypeslib.as_array(C.cast(tal, C.POINTER(C.c_uint32)), shape=(count, 4)).copy())
            return 0

        cb = LD_SINK(_cb)
        self._check(call(cb))
        assert int(total.value) == sum(self.last_ld_calls)

        def cat(p, shape):
            return np.concatenate(p) if p else np.zeros(shape, np.uint32)

        return cat(parts[0], 0), cat(parts[1], 0), cat(parts[2], (0, 4)), a

    def nearest_windows(self, measure, windows, k: int, square: bool = True, row_slot: int = 0, col_slot: int = 1,
                        row_begin: int = 0, row_end: int | None = None, tallies: bool = False, max_entries: int = 0):
        """The k nearest records of every row record in every column window (dst_nearest_windows):
        (index[n_rows, n_windows, k_used], values[n_rows, n_windows, k_used]), plus tallies[..., width] when asked.  Per
        (row, window) ascending by (key of the window's value, index); square: slot 0 against itself without the diagonal,
        the canonical pair's value; else rows [row_begin, row_end) of row_slot against every record of col_slot.
        max_entries: the most pair-windows of one device slab (0: the default); the result does not depend on it."""
        m = _measure_id(measure)
        begin, end, nw = _window_arrays(windows)
        n_rows, _ = self.set_info(0 if square else row_slot)
        n_cols, _ = self.set_info(0 if square else col_slot)
        row_end = n_rows if row_end is None else row_end
        rows = max(row_end - row_begin, 0)
        ku = min(int(k), max(n_cols - 1, 0) if square else n_cols) if 1 <= int(k) <= 256 else 0
        width = self._lib.dst_tally_width(m)
        index = np.zeros((rows, nw, ku), np.uint32)
        values = np.zeros((rows, nw, ku), np.int64 if m in (0, 1) else np.float64)
        tal = np.zeros((rows, nw, ku, width), np.uint32) if tallies else None
        k_used = C.c_uint32()
        self._check(self._lib.dst_nearest_windows(self._h, m, int(square), row_slot, col_slot, row_begin, row_end,
                                                  begin.ctypes.data, end.ctypes.data, nw, int(k), int(max_entries),
                                                  index.ctypes.data, None if tal is None else tal.ctypes.data,
                                                  values.ctypes.data, rows * nw * ku, C.byref(k_used)))
        assert k_used.value == ku
        return (index, values, tal) if tallies else (index, values)

    def summary(self, measure, threshold: float = 0.0, square: bool = True, row_slot: int = 0, col_slot: int = 1,
                max_pairs: int = 0, bins: int = 0, width: float = 1.0, per_record: bool = True) -> dict:
        """Per-record and histogram summaries of the pairwise distances (dst_summary), a dict: `within` (uint32[n_rows], the
        partners within `threshold` by dst_clusters' rule), `summable` (uint32[n_rows], the partners whose value is not
        NaN and below 2^25) and `sum` (float64[n_rows], the exact fixed-point sum of their values, rounded once) unless
        per_record is False; `hist` (uint64[bins], bin b = values in [b width, (b + 1) width), the last bin open-ended,
        NaN in none) when bins > 0; and the totals `pairs`, `nan_pairs`, `summable_pairs`, `links`, `total_sum`, every pair once.
        square: slot 0, every pair counts for both of its records; else the records of row_slot against those of col_slot.
        max_pairs: the most pairs of one row slab (0: the default); the result does not depend on it."""
        m = _measure_id(measure)
        n_rows, _ = self.set_info(0 if square else row_slot)
        bins = int(bins)
        cap = max(n_rows, 1)
        within = np.zeros(cap, np.uint32) if per_record else None
        summable = np.zeros(cap, np.uint32) if per_record else None
        sums = np.zeros(cap, np.float64) if per_record else None
        hist = np.zeros(max(bins, 1), np.uint64) if bins else None
        tot = SummaryTotals()

        def ptr(a):
            return None if a is None else a.ctypes.data

        self._check(self._lib.dst_summary(self._h, m, int(square), row_slot, col_slot, float(threshold), int(max_pairs), bins,
                                          float(width), ptr(hist), ptr(within), ptr(summable), ptr(sums), n_rows, C.byref(tot)))
        out = {"pairs": int(tot.pairs), "nan_pairs": int(tot.nan_pairs), "summable_pairs": int(tot.summable_pairs),
               "links": int(tot.links), "total_sum": float(tot.sum)}
        if per_record:
            out.update(within=within[:n_rows], summable=summable[:n_rows], sum=sums[:n_rows])
        if bins:
            out["hist"] = hist[:bins]
        return out

    def window_summary(self, measure, windows, threshold: float = 0.0, square: bool = True, row_slot: int = 0,
                       col_slot: int = 1, per_record: bool = True) -> dict:
        """summary()'s counts and sums inside every column window [begin, end) of `windows` ((n_windows, 2) integers), reduced
        next to the window sweep (dst_window_summary): a dict of `within`, `summable` (uint32) and `sum` (float64), each of
        shape (n_windows, n_rows), unless per_record is False; and the totals `pairs`, `nan_pairs`, `summable_pairs`,
        `links` (uint64) and `total_sum` (float64), each of shape (n_windows,).  Window w's entries are bitwise summary()'s
        definition applied to run_windows(...)[w].  square: slot 0, every pair counts for both of its records; else the
        records of row_slot against those of col_slot."""
        m = _measure_id(measure)
        begin, end, nw = _window_arrays(windows)
        n_rows, _ = self.set_info(0 if square else row_slot)
        entries = nw * n_rows
        cap = max(entries, 1)
        within = np.zeros(cap, np.uint32) if per_record else None
        summable = np.zeros(cap, np.uint32) if per_record else None
        sums = np.zeros(cap, np.float64) if per_record else None
        tot = (SummaryTotals * max(nw, 1))()

        def ptr(a):
            return None if a is None else a.ctypes.data

        self._check(self._lib.dst_window_summary(self._h, m, int(square), row_slot, col_slot, begin.ctypes.data,
                                                 end.ctypes.data, nw, float(threshold), C.addressof(tot), ptr(within),
                                                 ptr(summable), ptr(sums), entries))
        t = np.frombuffer(tot, dtype=np.dtype([("pairs", np.uint64), ("nan_pairs", np.uint64), ("summable_pairs", np.uint64),
                                               ("links", np.uint64), ("sum", np.float64)]))[:nw]
        out = {"pairs": t["pairs"].copy(), "nan_pairs": t["nan_pairs"].copy(), "summable_pairs": t["summable_pairs"].copy(),
               "links": t["links"].copy(), "total_sum": t["sum"].copy()}
        if per_record:
            out.update(within=within[:entries].reshape(nw, n_rows), summable=summable[:entries].reshape(nw, n_rows),
                       sum=sums[:entries].reshape(nw, n_rows))
        return out

    def _group_labels(self, groups, n_groups, square, row_slot, col_slot, col_groups, n_col_groups):
        """The label arrays (uint32, -1 as DST_GROUP_NONE) and group counts of both sides, for group_summary() and
        window_group_summary()."""
        n_rows, _ = self.set_info(0 if square else row_slot)

        def labels(g, n, count, side):
            g = np.asarray(g)
            if g.ndim != 1 or len(g) != n or not np.issubdtype(g.dtype, np.integer):
                raise ValueError(f"{side} must be a 1-D integer array with one label per record ({n})")
            g64 = g.astype(np.int64)
            g64 = np.where(g64 == -1, GROUP_NONE, g64)
            if ((g64 < 0) | (g64 > GROUP_NONE)).any():
                raise ValueError(f"{side}: a label is neither -1 nor a 32-bit unsigned value")
            if count is None:
                assigned = g64[g64 != GROUP_NONE]
                count = int(assigned.max()) + 1 if len(assigned) else 1
            return np.ascontiguousarray(g64.astype(np.uint32)), int(count)

        rg, Gr = labels(groups, n_rows, n_groups, "groups")
        if square:
            cg, Gc = rg, Gr
        else:
            if col_groups is None:
                raise ValueError("the rectangle form needs col_groups")
            cg, Gc = labels(col_groups, self.set_info(col_slot)[0], n_col_groups, "col_groups")
        for count in (Gr, Gc):
            if not 0 <= count <= GROUP_NONE:
                raise ValueError("a group count must fit 32 bits")
        return rg, Gr, cg, Gc

    def group_summary(self, measure, groups, n_groups=None, threshold: float = float("inf"), square: bool = True,
                      row_slot: int = 0, col_slot: int = 1, col_groups=None, n_col_groups=None, max_pairs: int = 0,
                      per_record: bool = False) -> dict:
        """dst_summary's sums keyed by group (dst_group_summary).  `groups`: one integer label per row record (square: per
        record of slot 0), -1 or 2^32-1 for a record that belongs to no group; n_groups defaults to the largest label + 1.
        A rectangle takes col_groups / n_col_groups for the column set too.  Returns a dict of (G_r, G_c) arrays: `pairs`,
        `nan_pairs`, `summable_pairs`, `links` (uint64), `sum` (float64, the exact fixed-point sum rounded once), `min` and
        `max` (int64 or float64 by measure; NaN, or 0 for n / n_high, in a cell without a pair that is not NaN).  The square
        stores both orders of a cell; cell (a, a) holds the pairs inside a.  per_record=True adds `rec_within`,
        `rec_summable` (uint32) and `rec_sum` (float64) of shape (n_rows, G_c): dst_summary's per-record results restricted
        to the partners in each group, for every row record, assigned or not."""
        m = _measure_id(measure)
        n_rows, _ = self.set_info(0 if square else row_slot)
        rg, Gr, cg, Gc = self._group_labels(groups, n_groups, square, row_slot, col_slot, col_groups, n_col_groups)
        cells = (GroupCell * max(Gr * Gc, 1))()
        n_rec = n_rows * Gc
        within = np.zeros(max(n_rec, 1), np.uint32) if per_record else None
        summable = np.zeros(max(n_rec, 1), np.uint32) if per_record else None
        sums = np.zeros(max(n_rec, 1), np.float64) if per_record else None

        def ptr(a):
            return None if a is None else a.ctypes.data

        self._check(self._lib.dst_group_summary(self._h, m, int(square), row_slot, col_slot, rg.ctypes.data, Gr,
                                                None if square else cg.ctypes.data, Gc, float(threshold), int(max_pairs),
                                                C.addressof(cells), Gr * Gc, ptr(within), ptr(summable), ptr(sums), n_rec))
        raw = np.frombuffer(cells, dtype=np.uint64, count=Gr * Gc * 7).reshape(Gr, Gc, 7)
        value = np.int64 if m in (0, 1) else np.float64
        out = {"pairs": raw[:, :, 0].copy(), "nan_pairs": raw[:, :, 1].copy(), "summable_pairs": raw[:, :, 2].copy(),
               "links": raw[:, :, 3].copy(), "sum": raw[:, :, 4].copy().view(np.float64),
               "min": raw[:, :, 5].copy().view(value), "max": raw[:, :, 6].copy().view(value)}
        if per_record:
            out.update(rec_within=within[:n_rec].reshape(n_rows, Gc), rec_summable=summable[:n_rec].reshape(n_rows, Gc),
                       rec_sum=sums[:n_rec].reshape(n_rows, Gc))
        return out

    def window_group_summary(self, measure, windows, groups, n_groups=None, threshold: float = float("inf"), square: bool = True,
                             row_slot: int = 0, col_slot: int = 1, col_groups=None, n_col_groups=None,
                             per_record: bool = False) -> dict:
        """group_summary()'s cells inside every column window [begin, end) of `windows` ((n_windows, 2) integers), reduced
        next to the window sweep (dst_window_group_summary).  Labels as for group_summary(), at most WINDOW_GROUPS_MAX groups
        of one side.  Returns group_summary()'s keys with a leading window axis: `pairs`, `nan_pairs`, `summable_pairs`,
        `links`, `sum`, `min`, `max` of shape (n_windows, G_r, G_c), and with per_record=True `rec_within`, `rec_summable`
        and `rec_sum` of shape (n_windows, n_rows, G_c).  Window w's entries are bitwise group_summary()'s definition
        applied to run_windows(...)[w]."""
        m = _measure_id(measure)
        begin, end, nw = _window_arrays(windows)
        n_rows, _ = self.set_info(0 if square else row_slot)
        rg, Gr, cg, Gc = self._group_labels(groups, n_groups, square, row_slot, col_slot, col_groups, n_col_groups)
        n_cells = nw * Gr * Gc
        cells = (GroupCell * max(n_cells, 1))()
        n_rec = nw * n_rows * Gc
        within = np.zeros(max(n_rec, 1), np.uint32) if per_record else None
        summable = np.zeros(max(n_rec, 1), np.uint32) if per_record else None
        sums = np.zeros(max(n_rec, 1), np.float64) if per_record else None

        def ptr(a):
            return None if a is None else a.ctypes.data

        self._check(self._lib.dst_window_group_summary(self._h, m, int(square), row_slot, col_slot, begin.ctypes.data,
                                                       end.ctypes.data, nw, rg.ctypes.data, Gr,
                                                       None if square else cg.ctypes.data, Gc, float(threshold),
                                                       C.addressof(cells), n_cells, ptr(within), ptr(summable), ptr(sums), n_rec))
        raw = np.frombuffer(cells, dtype=np.uint64, count=n_cells * 7).reshape(nw, Gr, Gc, 7)
        value = np.int64 if m in (0, 1) else np.float64
        out = {"pairs": raw[..., 0].copy(), "nan_pairs": raw[..., 1].copy(), "summable_pairs": raw[..., 2].copy(),
               "links": raw[..., 3].copy(), "sum": raw[..., 4].copy().view(np.float64),
               "min": raw[..., 5].copy().view(value), "max": raw[..., 6].copy().view(value)}
        if per_record:
            out.update(rec_within=within[:n_rec].reshape(nw, n_rows, Gc), rec_summable=summable[:n_rec].reshape(nw, n_rows, Gc),
                       rec_sum=sums[:n_rec].reshape(nw, n_rows, Gc))
        return out

    def mst(self, measure, max_pairs: int = 0, tallies: bool = False):
        """Minimum spanning forest of slot 0 (dst_mst): (edges uint32[n_edges, 2], values[n_edges], rounds), plus
        tallies[n_edges, width] when asked.  An edge for every pair whose DST_OUT_DISTANCE payload is not NaN, ordered by
        (key of the value, i, j); the result is the unique minimum spanning forest under that order, its edges ascending,
        values bitwise run_square's.  rounds: the Boruvka rounds that added edges.  max_pairs: the most pairs of one row
        slab (0: the default); the result does not depend on it."""
        m = _measure_id(measure)
        n, _ = self.set_info(0)
        cap = max(n - 1, 1)
        width = self._lib.dst_tally_width(m)
        ei, ej = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
        values = np.zeros(cap, np.int64 if m in (0, 1) else np.float64)
        tal = np.zeros((cap, width), np.uint32) if tallies else None
        n_edges, rounds = C.c_uint64(), C.c_uint32()
        self._check(self._lib.dst_mst(self._h, m, int(max_pairs), ei.ctypes.data, ej.ctypes.data, values.ctypes.data,
                                      None if tal is None else tal.ctypes.data, cap, C.byref(n_edges), C.byref(rounds)))
        ne = int(n_edges.value)
        edges = np.stack([ei[:ne], ej[:ne]], axis=1)
        out = (edges, values[:ne].copy(), int(rounds.value))
        return out + (tal[:ne].copy(),) if tallies else out

    def nj(self, measure, max_pairs: int = 0):
        """Neighbour-joining tree of slot 0 (dst_nj): (parent uint32[2n-2], length float64[2n-2]).  Leaves are 0..n-1,
        the node made in round s is n + s, the root 2n - 3 (parent 0xFFFFFFFF, length 0).  max_pairs: the most pairs of
        one row slab of the fill (0: the default); the tree does not depend on it."""
        m = _measure_id(measure)
        n, _ = self.set_info(0)
        cap = max(2 * n - 2, 1)
        parent, length = np.zeros(cap, np.uint32), np.zeros(cap, np.float64)
        self._check(self._lib.dst_nj(self._h, m, int(max_pairs), parent.ctypes.data, length.ctypes.data, 2 * n - 2))
        return parent, length

    def nj_bootstrap(self, measure, codes, parent, replicates: int, seed: int = 1, max_pairs: int = 0,
                     trees: bool = False):
        """Bootstrap support of the main tree `parent` (dst_nj_bootstrap) from `replicates` column resamplings of
        `codes` (n x L uint8, host memory; slots 0 and 1 are not touched): support uint32[2n-2], the number of
        replicate trees that hold the split of each internal non-root node (0xFFFFFFFF at leaves and the root).
        trees=True: (support, replicate parents uint32[replicates, 2n-2])."""
        m = _measure_id(measure)
        codes = np.asarray(codes)
        if codes.dtype != np.uint8 or codes.ndim != 2:
            raise ValueError("codes must be a 2-D uint8 array")
        codes = np.ascontiguousarray(codes)
        n, L = codes.shape
        parent = np.ascontiguousarray(parent, np.uint32)
        N = max(2 * n - 2, 1)
        if len(parent) != 2 * n - 2:
            raise ValueError("parent needs 2n - 2 entries for n records")
        support = np.zeros(N, np.uint32)
        reps = np.zeros((max(int(replicates), 1), N), np.uint32) if trees else None
        self._check(self._lib.dst_nj_bootstrap(self._h, m, codes.ctypes.data, n, L, max(L, 1), int(replicates),
                                               int(seed) & 0xFFFFFFFFFFFFFFFF, int(max_pairs), parent.ctypes.data,
                                               support.ctypes.data, None if reps is None else reps.ctypes.data,
                                               2 * n - 2))
        return (support, reps) if trees else support

    def nj_matrix(self, d):
        """Neighbour-joining tree of an n x n distance matrix (dst_nj_matrix; only the strict upper triangle is read):
        (parent, length) as nj()."""
        d = np.ascontiguousarray(d, np.float64)
        if d.ndim != 2 or d.shape[0] != d.shape[1]:
            raise ValueError("nj_matrix needs a square matrix")
        n = d.shape[0]
        cap = max(2 * n - 2, 1)
        parent, length = np.zeros(cap, np.uint32), np.zeros(cap, np.float64)
        self._check(self._lib.dst_nj_matrix(self._h, d.ctypes.data, n, parent.ctypes.data, length.ctypes.data,
                                            max(2 * n - 2, 0)))
        return parent, length

    def dendrogram(self, measure, linkage="average", max_pairs: int = 0, stats: bool = False):
        """Dendrogram of slot 0 (dst_dendrogram) under linkage "average" (UPGMA), "weighted" (WPGMA) or "complete":
        (parent uint32[2n-1], length float64[2n-1], height float64[2n-1]).  Leaves are 0..n-1, the node made in round t
        is n + t, the root 2n - 2 (parent 0xFFFFFFFF, length 0).  max_pairs: the most pairs of one row slab of the fill
        (0: the default); the tree does not depend on it.  stats=True: also row_scans, the whole-row scans made."""
        m, link = _measure_id(measure), _linkage_id(linkage)
        n, _ = self.set_info(0)
        cap = max(2 * n - 1, 1)
        parent, length, height = np.zeros(cap, np.uint32), np.zeros(cap, np.float64), np.zeros(cap, np.float64)
        scans = C.c_uint64()
        self._check(self._lib.dst_dendrogram(self._h, m, link, int(max_pairs), parent.ctypes.data, length.ctypes.data,
                                             height.ctypes.data, max(2 * n - 1, 0), C.byref(scans)))
        return (parent, length, height, int(scans.value)) if stats else (parent, length, height)

    def dendrogram_matrix(self, d, linkage="average", stats: bool = False):
        """Dendrogram of an n x n distance matrix (dst_dendrogram_matrix; only the strict upper triangle is read):
        (parent, length, height) as dendrogram(), with row_scans when stats=True."""
        d = np.ascontiguousarray(d, np.float64)
        if d.ndim != 2 or d.shape[0] != d.shape[1]:
            raise ValueError("dendrogram_matrix needs a square matrix")
        link = _linkage_id(linkage)
        n = d.shape[0]
        cap = max(2 * n - 1, 1)
        parent, length, height = np.zeros(cap, np.uint32), np.zeros(cap, np.float64), np.zeros(cap, np.float64)
        scans = C.c_uint64()
        self._check(self._lib.dst_dendrogram_matrix(self._h, d.ctypes.data, n, link, parent.ctypes.data,
                                                    length.ctypes.data, height.ctypes.data, max(2 * n - 1, 0),
                                                    C.byref(scans)))
        return (parent, length, height, int(scans.value)) if stats else (parent, length, height)

    # ---- runs into device memory (bench / multi-GPU) ------------------------------------------
    def run_square_device(self, measure, row_begin: int, row_end: int, d_out: int, capacity: int,
                          tallies: bool = False, stream: int | None = None, out_kind: int | None = None):
        m = _measure_id(measure)
        kind = out_kind if out_kind is not None else (OUT_TALLY if tallies else OUT_DISTANCE)
        self._check(self._lib.dst_run_square(self._h, m, row_begin, row_end, kind, d_out, capacity, stream))

    def finalize_device(self, measure, row_begin: int, row_end: int, d_tallies: int, d_out: int, capacity: int,
                        tally_kind: int = OUT_TALLY16, square: bool = True, row_slot: int = 0, col_slot: int = 0,
                        stream: int | None = None, close: bool = False):
        """Tallies already on this GPU (OUT_TALLY / OUT_TALLY16 layout) -> distances (dst_finalize_device).
        close: the text path's arithmetic (reference operation order, table logarithm) instead of the epilogue's."""
        m = _measure_id(measure)
        self._check(self._lib.dst_finalize_device(self._h, m, int(square), row_slot, col_slot, row_begin, row_end,
                                                  tally_kind | (FIN_CLOSE if close else 0), d_tallies, d_out, capacity, stream))

    def run_rect_device(self, measure, row_slot: int, col_slot: int, row_begin: int, row_end: int,
                        d_out: int, capacity: int, tallies: bool = False, stream: int | None = None,
                        out_kind: int | None = None):
        m = _measure_id(measure)
        kind = out_kind if out_kind is not None else (OUT_TALLY if tallies else OUT_DISTANCE)
        self._check(self._lib.dst_run_rect(self._h, m, row_slot, col_slot, row_begin, row_end, kind, d_out, capacity, stream))

    def set_prep_threshold(self, site_comparisons: float):
        """dst_set_prep_threshold: 0 sends every upload through the consensus path's fused preparation."""
        self._check(self._lib.dst_set_prep_threshold(self._h, float(site_comparisons)))

    def set_ids(self, slot: int, ids: list[str]):
        """Record ids of the packed set in `slot` (dst_set_ids), for the device-side TSV text."""
        blobs = [s.encode() for s in ids]
        offs = np.zeros(len(blobs) + 1, np.uint64)
        offs[1:] = np.cumsum([len(b) for b in blobs])
        chars = b"".join(blobs)
        self._check(self._lib.dst_set_ids(self._h, slot, chars, offs.ctypes.data_as(C.POINTER(C.c_uint64)), len(blobs)))

    def text_square(self, measure, row_begin: int, row_end: int, capacity: int = 1 << 26) -> bytes:
        """TSV lines of rows [row_begin, row_end) x later records, formatted on the GPU (dst_text_square)."""
        buf = C.create_string_buffer(capacity)
        n = C.c_size_t(0)
        self._check(self._lib.dst_text_square(self._h, _measure_id(measure), row_begin, row_end, C.addressof(buf), capacity,
                                              C.byref(n)))
        return buf.raw[:n.value]

    def text_rect(self, measure, row_slot: int, col_slot: int, row_begin: int, row_end: int, swap_ids: bool = False,
                  capacity: int = 1 << 26) -> bytes:
        buf = C.create_string_buffer(capacity)
        n = C.c_size_t(0)
        self._check(self._lib.dst_text_rect(self._h, _measure_id(measure), row_slot, col_slot, row_begin, row_end,
                                            int(swap_ids), C.addressof(buf), capacity, C.byref(n)))
        return buf.raw[:n.value]

    def text_matrix(self, measure, row_begin: int = 0, row_end: int | None = None, square: bool = True, row_slot: int = 0,
                    col_slot: int = 1, style: str | int = "tsv", capacity: int = 1 << 26) -> bytes:
        """Rows [row_begin, row_end) of a distance matrix, formatted on the GPU (dst_text_matrix): per row the id, then
        a separator ('\\t' for "tsv", ' ' for "phylip") and the value for every column, then '\\n'; no header line.
        square: slot 0 against itself, diagonal included; else row_slot x col_slot.  row_end None: every row."""
        if row_end is None:
            row_end = self.set_info(0 if square else row_slot)[0]
        st = MATRIX_STYLES[style] if isinstance(style, str) else int(style)
        buf = C.create_string_buffer(max(int(capacity), 1))
        n = C.c_size_t(0)
        self._check(self._lib.dst_text_matrix(self._h, _measure_id(measure), int(bool(square)), row_slot, col_slot,
                                              row_begin, row_end, st, C.addressof(buf), capacity, C.byref(n)))
        return buf.raw[:n.value]

    def text_stats(self) -> tuple[int, int]:
        """(values the device noted as near ties of the 12th decimal, how many of them the host printed differently)"""
        a, b = C.c_uint64(), C.c_uint64()
        self._check(self._lib.dst_text_stats(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def last_kernel_ms(self) -> dict:
        a, b, c = C.c_float(), C.c_float(), C.c_float()
        self._check(self._lib.dst_last_kernel_ms(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"pair_ms": a.value, "finalize_ms": b.value, "pack_ms": c.value}

    def kernel_ms_mean(self, reset: bool = True) -> dict:
        """Mean pair / pack kernel time over the launches since the last reset (HIP events on the launch stream, read once:
        dst_kernel_ms_mean)."""
        a, b, na, nb = C.c_float(), C.c_float(), C.c_int(), C.c_int()
        self._check(self._lib.dst_kernel_ms_mean(self._h, int(reset), C.byref(a), C.byref(na), C.byref(b), C.byref(nb)))
        return {"pair_ms": a.value, "pair_launches": na.value, "pack_ms": b.value, "pack_launches": nb.value}

    def out_bytes(self, measure, pairs: int, tallies: bool = False) -> int:
        return int(self._lib.dst_out_bytes(_measure_id(measure), OUT_TALLY if tallies else OUT_DISTANCE,
                                           pairs))


class Comm:
    """dst_comm: the ranks of a multi-GPU job (one process — or, in tests, one thread — per rank).

    Comm.rccl(eng, id_bytes, rank, world): RCCL inside the library (dst_comm_create); `id_bytes` comes from
    Comm.unique_id() on rank 0 and travels by the launcher's own means.
    Comm.custom(eng, rank, world, allgather): the caller's transport — allgather(d_send, d_recv, bytes_per_rank, stream)
    with raw device pointers (dst_comm_create_custom)."""

    def __init__(self, eng: Engine, handle, keep=None):
        self._eng, self._lib, self._h, self._keep = eng, eng._lib, handle, keep

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        rc = load().dst_comm_unique_id(buf, 128)
        if rc:
            raise DistanceError(rc, "dst_comm_unique_id (RCCL not available?)")
        return bytes(buf)

    @classmethod
    def rccl(cls, eng: Engine, id_bytes: bytes, rank: int, world: int) -> "Comm":
        h = C.c_void_p()
        buf = (C.c_uint8 * 128).from_buffer_copy(id_bytes)
        eng._check(eng._lib.dst_comm_create(eng._h, buf, rank, world, C.byref(h)))
        return cls(eng, h)

    @classmethod
    def custom(cls, eng: Engine, rank: int, world: int, allgather) -> "Comm":
        def _cb(_user, d_send, d_recv, nbytes, stream):
            try:
                allgather(d_send, d_recv, int(nbytes), stream)
                return 0
            except Exception as exc:   # an exception must not cross the C frames
                import traceback
                traceback.print_exception(exc)
                return 1

        cb = ALLGATHER_FN(_cb)
        h = C.c_void_p()
        eng._check(eng._lib.dst_comm_create_custom(eng._h, rank, world, cb, None, C.byref(h)))
        return cls(eng, h, keep=cb)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.dst_comm_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Stream:
    """dst_stream_*: stream()'s batches (src/lib.rs:269-365) through page-locked ring slots, H2D / compare / D2H
    overlapped.  push() copies a batch into the acquired buffer and submits it; pop() returns the oldest batch's
    results [streamed record][loaded record] (a copy)."""

    def __init__(self, eng: Engine, measure, max_records: int, depth: int, tallies: bool, nibbles: bool = False):
        self._eng, self._lib = eng, eng._lib
        self.nibbles = nibbles
        self._m = _measure_id(measure)
        self._kind = OUT_TALLY if tallies else OUT_DISTANCE
        self._n_loaded, self._len = eng.set_info(0)
        self.max_records, self.depth = max_records, depth
        self._h = self._open()

    def _open(self):
        h = C.c_void_p()
        self._eng._check(self._lib.dst_stream_open_wire(self._eng._h, self._m, self._kind, self.max_records, self.depth,
                                                        int(self.nibbles), C.byref(h)))
        return h

    def buffer(self, padded: bool = False):
        """(codes view (max_records, width) into the page-locked input buffer, counts view (max_records, 4));
        padded: the rows whole, (max_records, pitch) — the bytes behind a row's width that no result depends on"""
        p, pitch, cnt = C.c_void_p(), C.c_size_t(), C.c_void_p()
        self._eng._check(self._lib.dst_stream_acquire(self._h, C.byref(p), C.byref(pitch), C.byref(cnt)))
        raw = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(self.max_records, pitch.value))
        counts = np.ctypeslib.as_array(C.cast(cnt, C.POINTER(C.c_uint32)), shape=(self.max_records, 4))
        if padded:
            return raw, counts
        return raw[:, :((self._len + 1) // 2 if self.nibbles else self._len)], counts

    def submit(self, n_records: int, use_counts: bool = False):
        self._eng._check(self._lib.dst_stream_submit(self._h, n_records, int(use_counts)))

    @staticmethod
    def to_nibbles(codes: np.ndarray, pad: int = 15) -> np.ndarray:
        """Paradis codes (n, L) -> the 4-bit wire format (n, ceil(L / 2)): site 2k in the low nibble of byte k.
        pad: the unused high nibble of an odd width's last byte (ignored by the pack, whatever it holds)"""
        hi = np.ascontiguousarray(codes, np.uint8) >> 4
        if hi.shape[1] % 2:
            hi = np.concatenate([hi, np.full((hi.shape[0], 1), pad & 15, np.uint8)], axis=1)
        return hi[:, 0::2] | (hi[:, 1::2] << 4)

    def push(self, codes: np.ndarray, counts=None):
        buf, cbuf = self.buffer()
        buf[:len(codes)] = self.to_nibbles(codes) if self.nibbles else codes
        if counts is not None:
            cbuf[:len(codes)] = counts
        self.submit(len(codes), counts is not None)

    def in_flight(self) -> int:
        return int(self._lib.dst_stream_in_flight(self._h))

    def pop(self, copy: bool = True) -> np.ndarray:
        n, p = C.c_size_t(), C.c_void_p()
        self._eng._check(self._lib.dst_stream_collect(self._h, C.byref(n), C.byref(p)))
        if self._kind == OUT_TALLY:
            w = self._lib.dst_tally_width(self._m)
            arr = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=(n.value, self._n_loaded, w))
        elif self._m in (0, 1):
            arr = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int64)), shape=(n.value, self._n_loaded))
        else:
            arr = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_double)), shape=(n.value, self._n_loaded))
        return arr.copy() if copy else arr

    def close(self):
        if getattr(self, "_h", None):
            self._lib.dst_stream_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


CLOSEST_SIDES = {"loaded": 0, "streamed": 1}   # dst_closest_side


class ClosestStream(Stream):
    """dst_stream_open_closest: a Stream whose batches leave the k nearest records behind instead of the result matrix.
    side="loaded": pop() returns the batch's record count and result() the lists of the loaded records so far,
    index = streamed ordinals; side="streamed": pop() returns (index, values, tallies) of the batch's records, index =
    loaded records.  Ascending by (key of the value, index); values int64 for n / n_high, float64 otherwise."""

    def __init__(self, eng: Engine, measure, k: int, max_records: int, side="loaded", depth: int = 3, nibbles: bool = False):
        self.k = int(k)
        self.side = side
        self._side = CLOSEST_SIDES.get(side, side)
        if not isinstance(self._side, int):
            raise DistanceError(1, f"unknown side {side!r}: loaded or streamed")
        super().__init__(eng, measure, max_records, depth, True, nibbles)
        self._w = self._lib.dst_tally_width(self._m)
        self._vtype = np.int64 if self._m in (0, 1) else np.float64

    def _open(self):
        h = C.c_void_p()
        self._eng._check(self._lib.dst_stream_open_closest(self._eng._h, self._m, self.k, self._side, self.max_records,
                                                           self.depth, int(self.nibbles), C.byref(h)))
        return h

    def pop(self, copy: bool = True):
        n, p = C.c_size_t(), C.c_void_p()
        self._eng._check(self._lib.dst_stream_collect(self._h, C.byref(n), C.byref(p)))
        if self._side != 1:
            return n.value
        return self.closest_batch(n.value)

    def closest_batch(self, n_records: int):
        """(index, values, tallies) of the batch pop() collected last: copies (dst_stream_closest_batch)"""
        ip, tp, vp, ku = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint32()
        self._eng._check(self._lib.dst_stream_closest_batch(self._h, C.byref(ip), C.byref(tp), C.byref(vp), C.byref(ku)))
        k = ku.value
        if n_records * k == 0:
            return (np.zeros((n_records, k), np.uint32), np.zeros((n_records, k), self._vtype),
                    np.zeros((n_records, k, self._w), np.uint32))
        index = np.ctypeslib.as_array(C.cast(ip, C.POINTER(C.c_uint32)), shape=(n_records, k)).copy()
        vt = C.c_int64 if self._vtype is np.int64 else C.c_double
        values = np.ctypeslib.as_array(C.cast(vp, C.POINTER(vt)), shape=(n_records, k)).copy()
        tal = np.ctypeslib.as_array(C.cast(tp, C.POINTER(C.c_uint32)), shape=(n_records, k, self._w)).copy()
        return index, values, tal

    def next_index(self, n: int):
        """The ordinal of the next pushed record (dst_stream_closest_next_index)"""
        self._eng._check(self._lib.dst_stream_closest_next_index(self._h, int(n)))

    def result(self, tallies: bool = False, cap_entries: int | None = None):
        """side="loaded": (index[n_loaded, k_used], values[n_loaded, k_used][, tallies[n_loaded, k_used, width]]), a snapshot
        (dst_stream_closest_result); every pushed batch must have been popped."""
        cap = self._n_loaded * self.k if cap_entries is None else int(cap_entries)
        index = np.zeros(max(cap, 1), np.uint32)
        values = np.zeros(max(cap, 1), self._vtype)
        tal = np.zeros(max(cap, 1) * self._w, np.uint32) if tallies else None
        ku = C.c_uint32()
        self._eng._check(self._lib.dst_stream_closest_result(self._h, index.ctypes.data, None if tal is None else tal.ctypes.data,
                                                             values.ctypes.data, cap, C.byref(ku)))
        k, n = ku.value, self._n_loaded
        index, values = index[:n * k].reshape(n, k).copy(), values[:n * k].reshape(n, k).copy()
        if tallies:
            return index, values, tal[:n * k * self._w].reshape(n, k, self._w).copy()
        return index, values


class WindowClosestStream(Stream):
    """dst_stream_open_window_closest: a Stream whose batches leave, for every (loaded record, window), the k nearest
    streamed records behind.  pop() returns the batch's record count; result() the lists so far, index = streamed
    ordinals, ascending by (key of the window's value, ordinal); values int64 for n / n_high, float64 otherwise."""

    def __init__(self, eng: Engine, measure, windows, k: int, max_records: int, depth: int = 3, nibbles: bool = False,
                 max_entries: int = 0):
        self.k, self.max_entries = int(k), int(max_entries)
        self._begin, self._end, self.n_windows = _window_arrays(windows)
        super().__init__(eng, measure, max_records, depth, True, nibbles)
        self._w = self._lib.dst_tally_width(self._m)
        self._vtype = np.int64 if self._m in (0, 1) else np.float64

    def _open(self):
        h = C.c_void_p()
        self._eng._check(self._lib.dst_stream_open_window_closest(
            self._eng._h, self._m, self.k, self._begin.ctypes.data, self._end.ctypes.data, self.n_windows, self.max_entries,
            self.max_records, self.depth, int(self.nibbles), C.byref(h)))
        return h

    def pop(self, copy: bool = True):
        n, p = C.c_size_t(), C.c_void_p()
        self._eng._check(self._lib.dst_stream_collect(self._h, C.byref(n), C.byref(p)))
        return n.value

    def next_index(self, n: int):
        """The ordinal of the next pushed record (dst_stream_closest_next_index)"""
        self._eng._check(self._lib.dst_stream_closest_next_index(self._h, int(n)))

    def result(self, tallies: bool = False, counts: bool = False, cap_entries: int | None = None):
        """(index, values[, tallies][, counts]) shaped (n_loaded, n_windows, k_used[, width or 4]), a snapshot
        (dst_stream_window_closest_result); every pushed batch must have been popped.  counts (tn93): the listed streamed
        records' {A,T,G,C} inside the window, counted by code."""
        n, nw = self._n_loaded, self.n_windows
        cap = n * nw * self.k if cap_entries is None else int(cap_entries)
        index = np.zeros(max(cap, 1), np.uint32)
        values = np.zeros(max(cap, 1), self._vtype)
        tal = np.zeros(max(cap, 1) * self._w, np.uint32) if tallies else None
        cnt = np.zeros(max(cap, 1) * 4, np.uint32) if counts else None
        ku = C.c_uint32()
        self._eng._check(self._lib.dst_stream_window_closest_result(
            self._h, index.ctypes.data, None if tal is None else tal.ctypes.data, values.ctypes.data,
            None if cnt is None else cnt.ctypes.data, cap, C.byref(ku)))
        k = ku.value
        e = n * nw * k
        out = (index[:e].reshape(n, nw, k).copy(), values[:e].reshape(n, nw, k).copy())
        if tallies:
            out += (tal[:e * self._w].reshape(n, nw, k, self._w).copy(),)
        if counts:
            out += (cnt[:e * 4].reshape(n, nw, k, 4).copy(),)
        return out


class LinksStream(Stream):
    """dst_stream_open_links: a Stream whose batches leave the pairs within a threshold behind instead of the result matrix.
    pop() returns (n_records, streamed uint32[n], loaded uint32[n][, values[n]][, tallies[n, width]]): streamed = the
    record's index within the batch, loaded = the record of slot 0, streamed record outer, loaded record inner; values int64
    for n / n_high, float64 otherwise, bitwise the plain stream's; every window of the batch concatenated, as copies."""

    def __init__(self, eng: Engine, measure, threshold: float, max_records: int, depth: int = 3, nibbles: bool = False,
                 values: bool = True, tallies: bool = False, window: int = 0):
        self.threshold, self.values, self.tallies, self.window = float(threshold), bool(values), bool(tallies), int(window)
        super().__init__(eng, measure, max_records, depth, bool(tallies), nibbles)
        self._w = self._lib.dst_tally_width(self._m)
        self._vtype = np.int64 if self._m in (0, 1) else np.float64

    def _open(self):
        h = C.c_void_p()
        what = (LINKS_VALUES if self.values else 0) | (LINKS_TALLIES if self.tallies else 0)
        self._eng._check(self._lib.dst_stream_open_links(self._eng._h, self._m, self.threshold, what, self.window,
                                                         self.max_records, self.depth, int(self.nibbles), C.byref(h)))
        return h

    def links_batch(self, first: int = 0):
        """One window of the batch pop() collected last (dst_stream_links_batch): (batch_links, streamed, loaded[, values]
        [, tallies]) of the links from `first` on, as copies."""
        n, total = C.c_uint64(), C.c_uint64()
        sp, lp, vp, tp = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._eng._check(self._lib.dst_stream_links_batch(self._h, int(first), C.byref(n), C.byref(total), C.byref(sp),
                                                          C.byref(lp), C.byref(vp), C.byref(tp)))
        m = int(n.value)

        def arr(p, ctype, shape, dtype):
            if m == 0:
                return np.zeros(shape, dtype)
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(ctype)), shape=shape).view(dtype).copy()

        out = (int(total.value), arr(sp, C.c_uint32, (m,), np.uint32), arr(lp, C.c_uint32, (m,), np.uint32))
        if self.values:
            out += (arr(vp, C.c_int64, (m,), self._vtype),)
        if self.tallies:
            out += (arr(tp, C.c_uint32, (m, self._w), np.uint32),)
        return out

    def pop(self, copy: bool = True):
        n, p = C.c_size_t(), C.c_void_p()
        self._eng._check(self._lib.dst_stream_collect(self._h, C.byref(n), C.byref(p)))
        parts, first = None, 0
        while True:
            got = self.links_batch(first)
            parts = [[a] for a in got[1:]] if parts is None else [q + [a] for q, a in zip(parts, got[1:])]
            first += len(got[1])
            if first >= got[0]:
                break
        return (int(n.value),) + tuple(np.concatenate(q) if len(q) > 1 else q[0] for q in parts)

    def stats(self):
        """(links of every batch popped so far, windows written after collect) (dst_stream_links_stats)"""
        links, late = C.c_uint64(), C.c_uint64()
        self._eng._check(self._lib.dst_stream_links_stats(self._h, C.byref(links), C.byref(late)))
        return int(links.value), int(late.value)


class SummaryStream(Stream):
    """dst_stream_open_summary: a Stream whose batches leave summary()'s counts and exact sums behind instead of the result
    matrix.  pop() returns the batch's record count, or with streamed=True (n_records, within, summable, sum) of the batch's
    records over the loaded set, as copies; result() is summary()'s dict over every pair so far plus `records`: the totals,
    `within` / `summable` / `sum` of the loaded records when loaded=True, `hist` when bins > 0."""

    def __init__(self, eng: Engine, measure, max_records: int, threshold: float = 0.0, loaded: bool = True,
                 streamed: bool = False, bins: int = 0, width: float = 1.0, depth: int = 3, nibbles: bool = False):
        self.threshold, self.loaded, self.streamed = float(threshold), bool(loaded), bool(streamed)
        self.bins, self.width = int(bins), float(width)
        super().__init__(eng, measure, max_records, depth, False, nibbles)

    def _open(self):
        h = C.c_void_p()
        what = (STREAM_SUMMARY_LOADED if self.loaded else 0) | (STREAM_SUMMARY_STREAMED if self.streamed else 0)
        self._eng._check(self._lib.dst_stream_open_summary(self._eng._h, self._m, self.threshold, what, self.bins, self.width,
                                                           self.max_records, self.depth, int(self.nibbles), C.byref(h)))
        return h

    def summary_batch(self):
        """(n_records, within, summable, sum) of the batch pop() collected last: copies (dst_stream_summary_batch)"""
        n, wp, sp, dp = C.c_size_t(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._eng._check(self._lib.dst_stream_summary_batch(self._h, C.byref(n), C.byref(wp), C.byref(sp), C.byref(dp)))
        m = int(n.value)
        within = np.ctypeslib.as_array(C.cast(wp, C.POINTER(C.c_uint32)), shape=(m,)).copy()
        summable = np.ctypeslib.as_array(C.cast(sp, C.POINTER(C.c_uint32)), shape=(m,)).copy()
        sums = np.ctypeslib.as_array(C.cast(dp, C.POINTER(C.c_double)), shape=(m,)).copy()
        return m, within, summable, sums

    def pop(self, copy: bool = True):
        n, p = C.c_size_t(), C.c_void_p()
        self._eng._check(self._lib.dst_stream_collect(self._h, C.byref(n), C.byref(p)))
        return self.summary_batch() if self.streamed else int(n.value)

    def result(self, cap: int | None = None) -> dict:
        """A snapshot of everything kept so far (dst_stream_summary_result); every pushed batch must have been popped."""
        n = self._n_loaded
        cap = n if cap is None else int(cap)
        room = max(cap, 1)
        within = np.zeros(room, np.uint32) if self.loaded else None
        summable = np.zeros(room, np.uint32) if self.loaded else None
        sums = np.zeros(room, np.float64) if self.loaded else None
        hist = np.zeros(max(self.bins, 1), np.uint64) if self.bins else None
        tot, records = SummaryTotals(), C.c_uint64()

        def ptr(a):
            return None if a is None else a.ctypes.data

        self._eng._check(self._lib.dst_stream_summary_result(self._h, ptr(hist), ptr(within), ptr(summable), ptr(sums), cap,
                                                             C.byref(tot), C.byref(records)))
        out = {"records": int(records.value), "pairs": int(tot.pairs), "nan_pairs": int(tot.nan_pairs),
               "summable_pairs": int(tot.summable_pairs), "links": int(tot.links), "total_sum": float(tot.sum)}
        if self.loaded:
            out.update(within=within[:n], summable=summable[:n], sum=sums[:n])
        if self.bins:
            out["hist"] = hist[:self.bins]
        return out


class GroupSummaryStream(Stream):
    """dst_stream_open_group_summary: a Stream whose batches leave group_summary()'s sums behind instead of the result
    matrix.  push() takes the batch's labels (groups; None: all in streamed group 0; -1: no group).  pop() returns the batch's
    record count, or with streamed=True (n_records, within, summable, sum), each (n_records, G_l), as copies: the batch's
    records over the loaded groups.  result() is group_summary()'s cell keys of shape (G_s, G_l) over every record so far
    plus `records`, and with loaded=True `rec_within` / `rec_summable` / `rec_sum` of shape (n_loaded, G_s)."""

    def __init__(self, eng: Engine, measure, max_records: int, loaded_groups=None, n_loaded_groups=None,
                 n_streamed_groups: int = 1, threshold: float = float("inf"), loaded: bool = False, streamed: bool = False,
                 depth: int = 3, nibbles: bool = False):
        self.threshold, self.loaded, self.streamed = float(threshold), bool(loaded), bool(streamed)
        n_loaded, _ = eng.set_info(0)
        if loaded_groups is None:
            self._labels, self.n_loaded_groups = None, 1 if n_loaded_groups is None else int(n_loaded_groups)
        else:
            g = np.asarray(loaded_groups)
            if g.ndim != 1 or len(g) != n_loaded or not np.issubdtype(g.dtype, np.integer):
                raise ValueError(f"loaded_groups must be a 1-D integer array with one label per loaded record ({n_loaded})")
            self._labels = _group_labels_u32(g, "loaded_groups")
            if n_loaded_groups is None:
                assigned = self._labels[self._labels != GROUP_NONE]
                n_loaded_groups = int(assigned.max()) + 1 if len(assigned) else 1
            self.n_loaded_groups = int(n_loaded_groups)
        self.n_streamed_groups = int(n_streamed_groups)
        for count in (self.n_loaded_groups, self.n_streamed_groups):
            if not 0 <= count <= GROUP_NONE:
                raise ValueError("a group count must fit 32 bits")
        super().__init__(eng, measure, max_records, depth, False, nibbles)

    def _open(self):
        h = C.c_void_p()
        what = (STREAM_GROUPS_LOADED if self.loaded else 0) | (STREAM_GROUPS_STREAMED if self.streamed else 0)
        self._eng._check(self._lib.dst_stream_open_group_summary(
            self._eng._h, self._m, self.threshold, what, None if self._labels is None else self._labels.ctypes.data,
            self.n_loaded_groups, self.n_streamed_groups, self.max_records, self.depth, int(self.nibbles), C.byref(h)))
        return h

    def labels(self) -> np.ndarray:
        """The acquired buffer's label block (max_records,) uint32, zero-filled by buffer() (dst_stream_group_labels)"""
        p = C.c_void_p()
        self._eng._check(self._lib.dst_stream_group_labels(self._h, C.byref(p)))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=(self.max_records,))

    def push(self, codes: np.ndarray, counts=None, groups=None):
        buf, cbuf = self.buffer()
        buf[:len(codes)] = self.to_nibbles(codes) if self.nibbles else codes
        if counts is not None:
            cbuf[:len(codes)] = counts
        if groups is not None:
            g = np.asarray(groups)
            if g.ndim != 1 or len(g) != len(codes) or not np.issubdtype(g.dtype, np.integer):
                raise ValueError(f"groups must be a 1-D integer array with one label per record ({len(codes)})")
            self.labels()[:len(codes)] = _group_labels_u32(g, "groups")
        self.submit(len(codes), counts is not None)

    def group_summary_batch(self):
        """(n_records, within, summable, sum) of the batch pop() collected last: copies (dst_stream_group_summary_batch)"""
        n, wp, sp, dp = C.c_size_t(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._eng._check(self._lib.dst_stream_group_summary_batch(self._h, C.byref(n), C.byref(wp), C.byref(sp), C.byref(dp)))
        m, G = int(n.value), self.n_loaded_groups
        within = np.ctypeslib.as_array(C.cast(wp, C.POINTER(C.c_uint32)), shape=(m, G)).copy()
        summable = np.ctypeslib.as_array(C.cast(sp, C.POINTER(C.c_uint32)), shape=(m, G)).copy()
        sums = np.ctypeslib.as_array(C.cast(dp, C.POINTER(C.c_double)), shape=(m, G)).copy()
        return m, within, summable, sums

    def pop(self, copy: bool = True):
        n, p = C.c_size_t(), C.c_void_p()
        self._eng._check(self._lib.dst_stream_collect(self._h, C.byref(n), C.byref(p)))
        return self.group_summary_batch() if self.streamed else int(n.value)

    def result(self, cells_cap: int | None = None, rec_cap: int | None = None) -> dict:
        """A snapshot of everything kept so far (dst_stream_group_summary_result); every pushed batch must have been popped."""
        Gs, Gl, n = self.n_streamed_groups, self.n_loaded_groups, self._n_loaded
        n_cells, n_rec = Gs * Gl, n * Gs
        cells_cap = n_cells if cells_cap is None else int(cells_cap)
        rec_cap = n_rec if rec_cap is None else int(rec_cap)
        cells = (GroupCell * max(cells_cap, 1))()
        room = max(rec_cap, 1)
        within = np.zeros(room, np.uint32) if self.loaded else None
        summable = np.zeros(room, np.uint32) if self.loaded else None
        sums = np.zeros(room, np.float64) if self.loaded else None
        records = C.c_uint64()

        def ptr(a):
            return None if a is None else a.ctypes.data

        self._eng._check(self._lib.dst_stream_group_summary_result(self._h, C.addressof(cells), cells_cap, ptr(within), ptr(summable),
                                                                   ptr(sums), rec_cap, C.byref(records)))
        raw = np.frombuffer(cells, dtype=np.uint64, count=n_cells * 7).reshape(Gs, Gl, 7)
        value = np.int64 if self._m in (0, 1) else np.float64
        out = {"records": int(records.value), "pairs": raw[:, :, 0].copy(), "nan_pairs": raw[:, :, 1].copy(),
               "summable_pairs": raw[:, :, 2].copy(), "links": raw[:, :, 3].copy(), "sum": raw[:, :, 4].copy().view(np.float64),
               "min": raw[:, :, 5].copy().view(value), "max": raw[:, :, 6].copy().view(value)}
        if self.loaded:
            out.update(rec_within=within[:n_rec].reshape(n, Gs), rec_summable=summable[:n_rec].reshape(n, Gs),
                       rec_sum=sums[:n_rec].reshape(n, Gs))
        return out


def _group_labels_u32(g: np.ndarray, side: str) -> np.ndarray:
    """integer labels as uint32, -1 as DST_GROUP_NONE (Engine._group_labels' rule)"""
    g64 = g.astype(np.int64)
    g64 = np.where(g64 == -1, GROUP_NONE, g64)
    if ((g64 < 0) | (g64 > GROUP_NONE)).any():
        raise ValueError(f"{side}: a label is neither -1 nor a 32-bit unsigned value")
    return np.ascontiguousarray(g64.astype(np.uint32))
