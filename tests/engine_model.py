"""A host-side model of one Engine and a vocabulary of operations on it (used by test_gpu_sequences.py).

The README promises that an answer depends neither on the path nor on what the context did before.  DeviceSet and
dst_ctx keep about a dozen caches, each valid under a key of its own: the reference (ref.valid), the lists (rec.valid,
ref_owner, ref_epoch, without_hot), the pack's counts (pre_valid, pre_epoch), the run records (runs.active, corr_family),
the per-record constants (aconst_family, aconst_wide, aconst_ref_*), the hot columns (hot_epoch, hot_ref_*), deferred
planes (planes_deferred, lean), base counts (have_counts, text_counts_epoch), record ids, tile schedules, and the
grow-only scratch of text, nearest, clusters, NJ and bootstrap.  A wrong key shows only after a certain ORDER of calls.

Model holds what a caller knows (the bytes of each slot, the caller's base counts, the ids, the knobs) and says what
every operation must answer, from two sources that both have to hold:

 1. the oracle, on whole rows picked by the model (picked_rows): n / n_high / raw and every tally exactly, jc69 / k80 /
    tn93 within the finalisation bars of test_gpu_launch_variants.check_f64 (finalise_reference.exact on the oracle's
    tallies); base counts, the consensus and the difference lists exactly;
 2. a pristine engine, made for that one check, on the dense path, given the model's bytes and the same single
    operation: bit for bit (distances, tallies, text, nearest, clusters, NJ, bootstrap support, error statuses).  It has
    no history, so a difference is state that leaked.

An operation is a tuple (name, arguments...), so a failing sequence prints as a Python literal that replay() runs again.

The second vocabulary (ANALYSIS_OPS, walk_analyses; test_gpu_sequences_analyses.py) adds the analyses that came later —
mst, dendrogram, summary, group_summary, representatives, links, run_pairs, pair_sites, run_windows, window_base_counts,
nearest_windows — and dst_streams as handles: ("stream_open", tag, kind, measure, ...), ("stream_push", tag, kind of
codes, n, seed), ("stream_pop", tag), ("stream_result", tag, tallies[, cap_entries]), ("stream_close", tag).  The model
keeps every open stream's own history (ModelStream).  The rule: a stream's answers depend on that history and on slot 0,
and on nothing else the context did — each pop and each result is compared, bit for bit, with a pristine engine that was
given slot 0, the same stream and the same batches with nothing in between, and the lists of a closest stream (loaded
side) and of a window-closest stream also with the header's definition (Runner._stream_definition).  The analyses'
source 1 is the reference module of each, by the rule of its own test module (check_analysis).
"""
from __future__ import annotations

import functools

import numpy as np

ALL = ("n", "n_high", "raw", "jc69", "k80", "tn93")
PREP = {"zero": 0.0, "default": 2.0e10, "huge": 1e30}
PATH_NAMES = ("auto", "dense", "consensus", "hybrid")
KINDS = ("low", "clade", "runs", "clade_runs", "diverse", "uniform", "wide", "wide_clade")
ERR_ARG, ERR_INVALID_CODE, ERR_STATE, ERR_CAPACITY = 1, 3, 4, 6
CHUNK = 128          # kChunkSites
RUN_CHUNKS = 4       # a record with this many whole chunks of N is a run record (test_gpu_runs.py)
HOT_SHARE = 0.05     # kHotPermille

# the classes the walk's coverage is stated over; accessors of a set (consensus, differences, base counts) count as derived
CLASSES = ("upload", "knob", "square", "rect", "stream", "text", "derived", "error")
OP_CLASS = {
    "upload": "upload", "upload_device": "upload",
    "set_path": "knob", "set_prep": "knob", "set_variant": "knob", "set_ksplit": "knob",
    "run_square": "square", "run_square_device": "square", "run_slabs_square": "square",
    "run_rect": "rect", "run_slabs_rect": "rect",
    "run_stream_batch": "stream", "stream": "stream",
    "set_ids": "text", "text_square": "text", "text_rect": "text", "text_matrix": "text",
    "nearest": "derived", "clusters": "derived", "nj": "derived", "nj_bootstrap": "derived",
    "consensus": "derived", "differences": "derived", "base_counts": "derived",
    "bad_upload": "error", "err_text_capacity": "error", "err_width": "error", "err_nj_nonfinite": "error",
    "clusters_tiny_slabs": "error",
}
# operations only the directed sequences name (the walks draw from OP_CLASS, so the committed seeds stay the same walks)
DIRECTED_OPS = {"links": "derived", "pair_sites": "derived"}
# not operations of the library: what a directed sequence asserts about the engine's introspection
CHECKS = ("expect", "snapshot")

# The second vocabulary (test_gpu_sequences_analyses.py, walk_analyses): the analyses and stream kinds added since the
# first one, over classes of their own.  The uploads, knobs and pair runs are the first vocabulary's, drawn again so that
# the new calls meet them; links and pair_sites are listed here as well and stay in DIRECTED_OPS.
ANALYSIS_CLASSES = ("upload", "knob", "pair", "slab", "window", "pairlist", "handle", "error")
ANALYSIS_OPS = {
    "upload": "upload", "upload_device": "upload",
    "set_path": "knob", "set_prep": "knob", "set_variant": "knob", "set_ksplit": "knob",
    "run_square": "pair", "run_rect": "pair",
    "nearest": "slab", "mst": "slab", "dendrogram": "slab", "summary": "slab", "group_summary": "slab",
    "representatives": "slab", "links": "slab",
    "run_windows": "window", "window_base_counts": "window", "nearest_windows": "window",
    "run_pairs": "pairlist", "pair_sites": "pairlist",
    "stream_open": "handle", "stream_push": "handle", "stream_pop": "handle", "stream_result": "handle",
    "stream_close": "handle",
    "err_pairs_index": "error", "err_window": "error", "err_label": "error", "err_k": "error", "err_capacity": "error",
    "err_dendrogram_nonfinite": "error", "stream_push_bad": "error",
}
NEW_OPS = tuple(sorted(set(ANALYSIS_OPS) - set(OP_CLASS)))      # what the first vocabulary's walks never draw
STREAM_KINDS = ("plain", "closest_loaded", "closest_streamed", "links", "window_closest")
STREAM_OPS = ("stream_open", "stream_push", "stream_push_bad", "stream_pop", "stream_result", "stream_close")
LINKAGES = ("average", "weighted", "complete")


def op_class(op):
    return OP_CLASS.get(op[0]) or DIRECTED_OPS.get(op[0]) or ANALYSIS_OPS.get(op[0])


def analysis_class(op):
    return ANALYSIS_OPS.get(op[0])


# ------------------------------------------------------------------------------------------------ inputs
def make_codes(kind, n, L, seed):
    """The bytes of an upload: deterministic in (kind, n, L, seed).  (Kept for the few callers of one step: read only.)"""
    return _make_codes(str(kind), int(n), int(L), int(seed))


@functools.lru_cache(maxsize=6)
def _make_codes(kind, n, L, seed):
    from helpers import random_alignment, uniform_codes
    if kind == "uniform":
        return uniform_codes(n, L, seed)
    if kind == "diverse":
        return random_alignment(n, L, seed, divergence=0.3)
    import test_gpu_launch_variants as census
    if kind in ("wide", "wide_clade"):       # L >= 65,536: sparse enough for the lists
        codes = census.low_diversity(n, L, seed, subs=8e-4, p_n=1.5e-4, p_amb=5e-5)
    elif kind in ("runs", "clade_runs") and L >= 1024 and n >= 12:
        from tools import synth
        codes = synth.alignment(synth.SEED ^ seed, n, L)
        synth.apply_nruns(codes, synth.nrun_plan(seed, n, L, 0.08, 0.5))
        codes[1, :] = 240                                  # a record of nothing but N
        codes[2, CHUNK * 3:CHUNK * 6] = 244                # three whole chunks of gaps: below the threshold
        codes[3, 100:100 + CHUNK * 6 + 17] = 242           # unaligned: partial chunks at both ends
        codes[n - 2, L - 700:] = 240                       # to the end (the last chunk may be partial)
    else:
        codes = census.low_diversity(n, L, seed)
    if kind in ("clade", "clade_runs", "wide_clade") and n >= 3:
        codes = census.with_clade(codes, seed + 50)
    return np.ascontiguousarray(codes)


def caller_counts(n, seed):
    """base counts a caller brings (upper-case letters only in the reference: any numbers, not the codes' own)"""
    return np.random.default_rng(seed + 991).integers(1, 4000, size=(n, 4)).astype(np.uint32)


WINDOW_MENUS = ("all", "other", "few", "wide")


def window_list(L, which):
    """The window lists of an alignment of L sites, (n_windows, 2) uint64, every bound cut to L.
    "all" (9): the whole alignment, one site, an empty window, one inside the first 128-site chunk, one that ends at 128,
    one from 127 across 128 and 129, one that ends at L, one that overlaps the fourth, and the first again.
    "other" (9): nine other windows of the same kinds (cuts at 129 and 128, the empty one at L, the repeat in the middle).
    "few" (3).  "wide" (5, L > 65,536): across site 65,535 / 65,536, the site 65,535 alone, from 65,536 on, everything."""
    c = lambda x: min(max(int(x), 0), L)       # noqa: E731
    if which == "all":
        w = [(0, L), (c(63), c(64)), (c(5), c(5)), (c(3), c(100)), (c(100), c(128)), (c(127), c(300)), (c(L - 70), L),
             (c(50), c(200)), (0, L)]
    elif which == "other":
        w = [(c(1), L), (0, c(1)), (L, L), (c(130), c(250)), (c(64), c(129)), (c(128), c(129)), (c(L - 1), L), (c(60), c(140)),
             (c(130), c(250))]
    elif which == "few":
        w = [(0, L), (c(64), c(129)), (c(5), c(5))]
    elif which == "wide":
        assert L > 65_536
        w = [(65_000, c(66_000)), (65_535, 65_536), (65_536, L), (0, L), (60_000, 65_536)]
    else:
        raise ValueError(which)
    return np.array(w, np.uint64).reshape(len(w), 2)


def group_labels(n, n_groups, seed):
    """one label per record, drawn from (seed, n): about one record in ten belongs to no group (-1)"""
    rng = np.random.default_rng([seed, 0x6709, n])
    g = rng.integers(0, n_groups, n).astype(np.int64)
    g[rng.random(n) < 0.1] = -1
    return g


def pair_list(n_rows, n_cols, n_pairs, seed, square):
    """n_pairs (row, col) drawn from (seed, the sets' sizes); from four pairs on: a repeat, i > j, and — the square, an odd
    seed — i == j (a diagonal pair takes run_pairs' direct kernel whatever the route: an even seed keeps a list to the sweep)"""
    rng = np.random.default_rng([seed, 0x9A125])
    row, col = rng.integers(0, n_rows, n_pairs), rng.integers(0, n_cols, n_pairs)
    if n_pairs >= 4:
        row[1], col[1] = row[0], col[0]
        if square:
            row[3], col[3] = n_rows - 1, 0
            if seed % 2:
                col[2] = row[2]
            elif n_rows > 1:
                keep = row == col
                col[keep] = (row[keep] + 1) % n_rows
    return row.astype(np.uint32), col.astype(np.uint32)


def batch_codes(kind, n, L, seed, bad=False):
    """the bytes of a pushed batch; bad: one byte that is no code (7; its high nibble, 0, is none on the 4-bit wire either)"""
    codes = _batch(str(kind), int(n), int(L), int(seed))
    if bad:
        codes = codes.copy()
        codes[n // 2, L // 2] = 7
    return codes


@functools.lru_cache(maxsize=64)
def _batch(kind, n, L, seed):
    """(a stream's history is replayed at every check: its batches are kept apart from the uploads' six)"""
    return _make_codes.__wrapped__(kind, n, L, seed)


class ModelStream:
    """What the caller knows of one open dst_stream: how it was opened, against which upload of slot 0, and every batch
    pushed so far — its whole history, which with slot 0 is all its answers may depend on."""

    def __init__(self, op, slot0):
        self.op = op                      # ("stream_open", tag, kind, measure, ...)
        self.kind, self.measure = op[2], op[3]
        self.version, self.n, self.L = slot0.version, slot0.n, slot0.L
        self.depth = op[-1]
        self.history = []                 # (kind of codes, n, seed, bad, submitted)
        self.in_flight = []               # positions in history, oldest first
        self.popped = False               # a batch was collected since the last submit
        self.poisoned = False             # closest and window-closest streams: a collected batch held an invalid code


class Slot:
    def __init__(self, codes, counts, version):
        self.codes, self.counts, self.version = codes, counts, version
        self.n, self.L = codes.shape
        self._special = None
        self._true_counts = None

    def base_counts(self):
        """what tn93 divides by: the caller's, else counted from the codes (src/fastaio.rs:53-66)"""
        import oracle
        if self.counts is not None:
            return self.counts.astype(np.uint64)
        if self._true_counts is None:
            self._true_counts = oracle.count_bases_matrix(self.codes)
        return self._true_counts

    def special_rows(self):
        """records the engine may treat apart: nothing but N; run records (RUN_CHUNKS whole chunks of N-like codes and
        more); members of hot columns — records that carry another base than the plurality one at half or more of the
        columns where more than HOT_SHARE of the records do (a clade's defining substitutions; a run of N is no member).
        (More than half the columns hot: the engine never hands such a set to the hybrid path, and every record would be a
        member; then none is marked.)"""
        if self._special is None:
            c, n, L = self.codes, self.n, self.L
            nlike = (c >> 4) == 15
            rows = set(np.nonzero(nlike.all(axis=1))[0].tolist())
            nch = (L + CHUNK - 1) // CHUNK
            padded = np.ones((n, nch * CHUNK), bool)
            padded[:, :L] = nlike
            whole = padded.reshape(n, nch, CHUNK).all(axis=2).sum(axis=1)
            rows |= set(np.nonzero(whole >= RUN_CHUNKS)[0].tolist())
            if n >= 3:
                known = np.array([136, 72, 40, 24], np.uint8)
                votes = np.stack([(c == k).sum(axis=0) for k in known])
                plural = known[votes.argmax(axis=0)]
                sub = (c != plural[None, :]) & np.isin(c, known)
                hot = sub.mean(axis=0) > HOT_SHARE
                if 0 < hot.sum() * 2 <= L:
                    member = sub[:, hot].sum(axis=1) * 2 >= hot.sum()
                    rows |= set(np.nonzero(member)[0].tolist())
            self._special = rows
        return self._special


def picked_rows(slot, rb, re, square):
    """The rows of [rb, re) held to the oracle: the first and the last with a pair, every special record, and one row of
    every 64 (at a position that moves from block to block).  So at most 63 of every 64 rows are skipped, never a
    special one."""
    last = min(re, slot.n - 1 if square else slot.n) - 1
    if last < rb:
        return []
    rows = {rb, last} | {r for r in slot.special_rows() if rb <= r <= last}
    for k, block in enumerate(range(rb, last + 1, 64)):
        rows.add(min(block + (37 * (k + 1)) % 64, last))
    return sorted(rows)


class Model:
    def __init__(self):
        self.slot = [None, None]       # None: nothing uploaded, or the last upload was rejected
        self.ids = [None, None]
        self.path, self.prep, self.variant, self.ksplit = "auto", "default", 0, 0
        self.uploads = 0
        self._tally_cache = {}
        self.streams = {}              # tag -> ModelStream, the streams that are open

    def set_slot(self, k, codes, counts=None):
        self.uploads += 1
        self.slot[k] = Slot(codes, counts, self.uploads)
        live = {s.version for s in self.slot if s is not None}
        self._tally_cache = {key: v for key, v in self._tally_cache.items() if key[0] in live and key[1] in live}

    def ids_ok(self, k):
        return self.slot[k] is not None and self.ids[k] is not None and len(self.ids[k]) == self.slot[k].n

    def widths_differ(self, a, b):
        return self.slot[a].L != self.slot[b].L

    def oracle_tallies(self, measure, rows, cols, i):
        """tallies of record i of `rows` against every record of `cols` (the oracle's loops), kept per upload"""
        import oracle
        om = "n_high" if measure == "n" else "raw" if measure == "jc69" else measure
        key = (rows.version, cols.version, om, i)
        if key not in self._tally_cache:
            self._tally_cache[key] = oracle.tallies_rect(om, rows.codes[i:i + 1], cols.codes, threads=8)[0]
        return self._tally_cache[key]


# ------------------------------------------------------------------------------------------------ performing an operation
def id_list(tag, n):
    return ["%s%d" % (tag, k * 7919 % 100003) for k in range(n)]


def _window(n, rb, re):
    return rb, (n if re is None else re)


def _stream_batches(op, model):
    _, m, kind, total, batch, depth, seed, tallies, nibbles = op
    L = model.slot[0].L if model.slot[0] is not None else 100
    return make_codes(kind, total, L, seed), batch, depth


def perform(eng, op, model, caller_stream=None, streams=None):
    """Run `op` on `eng`; the result as plain data, or ("error", status).  Uploads and knobs return None.
    caller_stream: the Runner's streams, by number (Runner.caller_stream); streams: its open dst_streams, by tag."""
    import distance_amd as da
    try:
        return _perform(eng, op, model, caller_stream, streams)
    except da.DistanceError as exc:
        return ("error", exc.status)


def _perform(eng, op, model, caller_stream, streams=None):
    import distance_amd as da
    name = op[0]
    if name == "upload":
        _, slot, kind, n, L, seed, counts = op
        eng.upload(slot, make_codes(kind, n, L, seed), caller_counts(n, seed) if counts else None)
        return None
    if name == "upload_device":
        import torch
        _, slot, kind, n, L, seed, strided = op
        codes = make_codes(kind, n, L, seed)
        stride, off = (L + 3, 1) if strided else ((L + 127) // 128 * 128, 0)    # any stride and start / rows 128 bytes apart
        buf = torch.full((n * stride + 256,), 240, dtype=torch.uint8, device="cuda")
        rows = buf[off:off + n * stride].view(n, stride)
        rows[:, :L] = torch.from_numpy(codes).cuda()
        torch.cuda.synchronize()
        eng.upload_device(slot, buf.data_ptr() + off, n, L, stride)     # (waits for the pack on the context's stream)
        return None
    if name == "bad_upload":
        _, slot, n, L, seed = op
        codes = make_codes("low", n, L, seed).copy()
        codes[n // 2, L // 2] = 7
        eng.upload(slot, codes)
        return None
    if name == "set_path":
        return eng.set_path(op[1])
    if name == "set_prep":
        return eng.set_prep_threshold(PREP[op[1]])
    if name == "set_variant":
        return eng.set_variant(op[1])
    if name == "set_ksplit":
        return eng.set_ksplit(op[1])
    if name == "run_square":
        _, m, rb, re, tallies = op
        return eng.run_square(m, rb, re, tallies=tallies)
    if name == "run_square_device":
        import torch
        _, m, rb, re = op[:4]
        stream = caller_stream(op[4] if len(op) > 4 else 0)      # (name, measure, rows, [which of the caller's streams])
        n, _ = eng.set_info(0)
        pairs = da.square_row_start(n, re) - da.square_row_start(n, rb)
        out = torch.zeros(max(pairs, 1), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        eng.run_square_device(m, rb, re, out.data_ptr(), out.numel() * 8, stream=stream.cuda_stream)
        stream.synchronize()
        got = out[:pairs].cpu().numpy()
        return got.view(np.int64) if m in da.INT_MEASURES else got
    if name == "run_rect":
        _, m, rs, cs, rb, re, tallies = op
        return eng.run_rect(m, rs, cs, rb, re, tallies=tallies)
    if name in ("run_slabs_square", "run_slabs_rect"):
        _, m, rs, cs, max_pairs, tallies = op
        parts, firsts = [], []

        def sink(first, rb, re, arr):
            firsts.append((first, rb, re))
            parts.append(arr.copy())
        eng.set_info(rs), eng.set_info(cs)
        eng.run_slabs(m, sink, max_pairs, square=name == "run_slabs_square", row_slot=rs, col_slot=cs, tallies=tallies)
        assert [f[0] for f in firsts] == [int(x) for x in np.cumsum([0] + [len(p) for p in parts[:-1]])][:len(parts)], firsts   # in order, no gap
        return np.concatenate(parts) if parts else np.zeros(0)
    if name == "run_stream_batch":
        _, m, kind, nb, seed, tallies, counts = op
        L = model.slot[0].L if model.slot[0] is not None else 100
        return eng.run_stream_batch(m, make_codes(kind, nb, L, seed), caller_counts(nb, seed) if counts else None, tallies)
    if name == "stream":
        _, m, kind, total, batch, depth, seed, tallies, nibbles = op
        codes, batch, depth = _stream_batches(op, model)
        got = []
        with eng.stream(m, max_records=batch, depth=depth, tallies=tallies, nibbles=nibbles) as st:
            for b0 in range(0, total, batch):
                if st.in_flight() == depth - 1:
                    got.append(st.pop())
                st.push(codes[b0:b0 + batch])
            while st.in_flight():
                got.append(st.pop())
        return np.concatenate(got)
    if name == "consensus":
        return eng.consensus(op[1])
    if name == "differences":
        import oracle
        s = model.slot[op[1]]
        eng.set_info(op[1])
        lists = eng.differences(op[1], oracle.consensus(s.codes))
        return [np.array([len(x) for x in lists], np.int64), np.concatenate(lists) if lists else np.zeros(0, np.uint32)]
    if name == "base_counts":
        return eng.base_counts(op[1])
    if name == "set_ids":
        _, slot, tag = op
        n = model.slot[slot].n if model.slot[slot] is not None else 3
        eng.set_ids(slot, id_list(tag, n))
        return None
    if name == "text_square":
        _, m, rb, re = op
        return eng.text_square(m, rb, re, capacity=1 << 25)
    if name == "text_rect":
        _, m, rs, cs, rb, re, swap = op
        return eng.text_rect(m, rs, cs, rb, re, swap_ids=swap, capacity=1 << 25)
    if name == "text_matrix":
        _, m, square, rs, cs, rb, re, style = op
        return eng.text_matrix(m, rb, re, square=square, row_slot=rs, col_slot=cs, style=style, capacity=1 << 25)
    if name == "nearest":
        _, m, k, square, rs, cs = op
        return list(eng.nearest(m, k, square=square, row_slot=rs, col_slot=cs))
    if name == "links":
        _, m, thr, square, rs, cs, values, tallies = op[:8]      # (..., [max_pairs])
        return list(eng.links(m, thr, square=square, row_slot=rs, col_slot=cs, values=values, tallies=tallies,
                              max_pairs=op[8] if len(op) > 8 else 0))
    if name == "pair_sites":      # n_pairs pairs drawn from (seed, the sets' sizes): repeats and row == col among them
        _, m, n_pairs, square, rs, cs, seed = op
        n_rows, n_cols = eng.set_info(0 if square else rs)[0], eng.set_info(0 if square else cs)[0]
        rng = np.random.default_rng([seed, 0x51735])
        return list(eng.pair_sites(m, rng.integers(0, n_rows, n_pairs), rng.integers(0, n_cols, n_pairs), square=square,
                                   row_slot=rs, col_slot=cs))
    if name == "clusters":
        _, m, thr = op
        labels, links = eng.clusters(m, thr)
        return [labels, links]
    if name == "clusters_tiny_slabs":     # max_pairs = 1: every row a slab of its own (no error: the same clusters)
        _, m, thr = op
        labels, links = eng.clusters(m, thr, max_pairs=1)
        return [labels, links]
    if name in ("nj", "err_nj_nonfinite"):
        return list(eng.nj(op[1]))
    if name == "nj_bootstrap":
        _, m, reps, seed = op
        parent, length = eng.nj(m)
        support = eng.nj_bootstrap(m, model.slot[0].codes, parent, reps, seed=seed)
        return [parent, length, support]
    if name == "err_text_capacity":
        return eng.text_square(op[1], 0, min(2, eng.set_info(0)[0]), capacity=8)
    if name == "err_width":
        s = model.slot[op[1]]
        eng.set_info(op[1])
        return eng.differences(op[1], np.full(s.L + 1, 136, np.uint8))
    if name in ANALYSIS_OPS:
        return _perform_analysis(eng, op, model, streams)
    raise ValueError("unknown operation %r" % (op,))


def _sizes(eng, square, rs, cs):
    return eng.set_info(0 if square else rs), eng.set_info(0 if square else cs)


def summary_width(measure):
    return 4.0 if measure in ("n", "n_high") else 2.0 ** -6


def _perform_analysis(eng, op, model, streams):
    """the second vocabulary: results as lists of arrays (dicts as sorted (key, value) lists), stream handles by tag"""
    name = op[0]
    if name == "mst":
        _, m, max_pairs, tallies = op
        return list(eng.mst(m, max_pairs=max_pairs, tallies=tallies))
    if name in ("dendrogram", "err_dendrogram_nonfinite"):
        m, linkage, max_pairs = (op[1], op[2], op[3]) if name == "dendrogram" else (op[1], "average", 0)
        return list(eng.dendrogram(m, linkage, max_pairs=max_pairs))
    if name == "summary":
        _, m, thr, square, rs, cs, max_pairs, bins = op
        res = eng.summary(m, thr, square=square, row_slot=rs, col_slot=cs, max_pairs=max_pairs, bins=bins, width=summary_width(m))
        return [[k, res[k]] for k in sorted(res)]
    if name == "group_summary":
        _, m, G, seed, thr, square, rs, cs, max_pairs = op
        (nr, _), (nc, _) = _sizes(eng, square, rs, cs)
        res = eng.group_summary(m, group_labels(nr, G, seed), G, thr, square=square, row_slot=rs, col_slot=cs,
                                col_groups=None if square else group_labels(nc, 3, seed + 1), n_col_groups=None if square else 3,
                                max_pairs=max_pairs, per_record=True)
        return [[k, res[k]] for k in sorted(res)]
    if name == "representatives":
        _, m, thr, max_pairs, values, tallies = op
        return list(eng.representatives(m, thr, max_pairs=max_pairs, values=values, tallies=tallies))
    if name == "run_pairs":
        _, m, n_pairs, square, rs, cs, seed, values, tallies, max_pairs, route = op
        (nr, _), (nc, _) = _sizes(eng, square, rs, cs)
        row, col = pair_list(nr, nc, n_pairs, seed, square)
        got = eng.run_pairs(m, row, col, square=square, row_slot=rs, col_slot=cs, values=values, tallies=tallies, route=route,
                            max_pairs=max_pairs)
        return list(got) if isinstance(got, tuple) else [got]
    if name == "run_windows":
        _, m, which, square, rs, cs, rb, re, tallies = op
        L = eng.set_info(0 if square else rs)[1]
        return eng.run_windows(m, window_list(L, which), square=square, row_slot=rs, col_slot=cs, row_begin=rb, row_end=re,
                               tallies=tallies)
    if name == "window_base_counts":
        _, slot, which = op
        return eng.window_base_counts(slot, window_list(eng.set_info(slot)[1], which))
    if name == "nearest_windows":
        _, m, which, k, square, rs, cs, tallies, max_entries = op
        L = eng.set_info(0 if square else rs)[1]
        return list(eng.nearest_windows(m, window_list(L, which), k, square=square, row_slot=rs, col_slot=cs, tallies=tallies,
                                        max_entries=max_entries))
    if name == "err_pairs_index":       # the first index past the set
        n = eng.set_info(0)[0]
        return eng.run_pairs(op[1], [0, n], [0, 0])
    if name == "err_window":            # begin > end, or end > L
        L = eng.set_info(0)[1]
        bad = (5, 3) if op[1] == "reversed" else (0, L + 1)
        return eng.run_windows("n", np.array([(0, L), bad], np.uint64), tallies=True)
    if name == "err_label":             # a label that is not below the group count
        n = eng.set_info(0)[0]
        g = np.arange(n) % 3
        g[n - 1] = 3
        res = eng.group_summary(op[1], g, 3, 0.01)
        return [[k, res[k]] for k in sorted(res)]
    if name == "err_k":
        return list(eng.nearest_windows(op[1], window_list(eng.set_info(0)[1], "few"), op[2]))
    if name == "err_capacity":          # room for one entry where n x 3 windows x 1 are due: the buffers are whole all the same
        import ctypes as C
        from distance_amd.engine import _measure_id, _window_arrays
        n, L = eng.set_info(0)
        begin, end, nw = _window_arrays(window_list(L, "few"))
        index, values, ku = np.zeros((n, nw, 1), np.uint32), np.zeros((n, nw, 1), np.float64), C.c_uint32()
        eng._check(eng._lib.dst_nearest_windows(eng._h, _measure_id(op[1]), 1, 0, 1, 0, n, begin.ctypes.data, end.ctypes.data, nw, 1,
                                                0, index.ctypes.data, None, values.ctypes.data, 1, C.byref(ku)))
        return [index, values]
    return _perform_stream(eng, op, model, streams)


def open_stream(eng, op, L):
    """the stream object of ("stream_open", tag, kind, measure, ..., nibbles, max_records, depth)"""
    _, _tag, kind, m = op[:4]
    nibbles, max_records, depth = op[-3:]
    a = op[4:-3]
    if kind == "plain":          # (tallies,)
        return eng.stream(m, max_records, depth, a[0], nibbles)
    if kind in ("closest_loaded", "closest_streamed"):      # (k,)
        return eng.closest_stream(m, a[0], max_records, side=kind[8:], depth=depth, nibbles=nibbles)
    if kind == "links":          # (threshold, values, tallies, window)
        return eng.links_stream(m, a[0], max_records, depth, nibbles, a[1], a[2], a[3])
    if kind == "window_closest":  # (menu, k, max_entries)
        return eng.window_closest_stream(m, window_list(L, a[0]), a[1], max_records, depth, nibbles, a[2])
    raise ValueError(op)


def _plain(x):
    return list(x) if isinstance(x, tuple) else x


def _perform_stream(eng, op, model, streams):
    name, tag = op[0], op[1]
    if name == "stream_open":
        assert tag not in streams, ("tag in use", tag)
        streams[tag] = open_stream(eng, op, eng.set_info(0)[1])
        return None
    st = streams[tag]
    if name in ("stream_push", "stream_push_bad"):
        _, _, kind, n, seed = op
        st.push(batch_codes(kind, n, model.streams[tag].L, seed, bad=name == "stream_push_bad"))
        return None
    if name == "stream_pop":
        return _plain(st.pop())
    if name == "stream_result":      # (name, tag, tallies[, cap_entries])
        return list(st.result(tallies=op[2], cap_entries=op[3] if len(op) > 3 else None))
    if name == "stream_close":
        streams.pop(tag).close()
        return None
    raise ValueError("unknown operation %r" % (op,))


def same(a, b):
    """bit for bit (NaN equal to NaN), through lists and tuples"""
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray) and isinstance(b, np.ndarray):
        return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
    return type(a) is type(b) and a == b


# ------------------------------------------------------------------------------------------------ what the model expects
def expected_error(op, model):
    """The status `op` must fail with, None when it must succeed, "either" where the model leaves it to the pristine
    engine.  A slot whose last upload was rejected is not loaded (pinned: dst_api.cpp's shape_set clears `loaded` before the
    pack looks at the bytes, so every use is a clean DST_ERR_STATE until the next accepted upload; the other slot answers)."""
    name = op[0]
    s = model.slot
    if name in ANALYSIS_OPS and name not in OP_CLASS and name not in DIRECTED_OPS:
        return _expected_error_analysis(op, model)
    need = {"run_square": (0,), "run_square_device": (0,), "run_slabs_square": (0,), "text_square": (0,), "clusters": (0,),
            "clusters_tiny_slabs": (0,), "nj": (0,), "nj_bootstrap": (0,), "err_nj_nonfinite": (0,), "err_text_capacity": (0,),
            "stream": (0,), "consensus": (0,), "run_stream_batch": (0,)}
    if name in ("upload", "upload_device", "set_path", "set_prep", "set_variant", "set_ksplit", "set_ids"):
        return None
    if name == "bad_upload":
        return ERR_INVALID_CODE
    if name in ("run_rect", "run_slabs_rect"):
        slots = (op[2], op[3])
    elif name == "text_rect":
        slots = (op[2], op[3])
    elif name == "text_matrix":      # (name, measure, square, row slot, col slot, ...)
        slots = (0,) if op[2] else (op[3], op[4])
    elif name in ("nearest", "links", "pair_sites"):     # (name, measure, k / threshold / pairs, square, row slot, col slot, ...)
        slots = (0,) if op[3] else (op[4], op[5])
    elif name in ("differences", "base_counts", "err_width"):
        slots = (op[1],)
    else:
        slots = need[name]
    if any(s[k] is None for k in slots):
        return ERR_STATE
    if name in ("nearest", "links", "pair_sites") and not op[3] and slots[0] == slots[1]:
        return ERR_ARG
    if name == "text_matrix" and not op[2] and slots[0] == slots[1]:
        return ERR_ARG
    if len(slots) == 2 and model.widths_differ(*slots):
        return ERR_STATE
    if name == "consensus" and op[1] and s[1] is not None and s[1].L != s[0].L:
        return ERR_STATE
    if name in ("text_square", "text_rect", "text_matrix", "err_text_capacity") and not all(model.ids_ok(k) for k in slots):
        return ERR_STATE
    if name == "err_text_capacity":
        return ERR_CAPACITY if s[0].n >= 2 else None
    if name == "err_width":
        return ERR_STATE
    if name in ("nj", "nj_bootstrap", "err_nj_nonfinite"):
        if s[0].n < 3:
            return ERR_ARG
        if name == "err_nj_nonfinite":
            return ERR_STATE       # (a sequence names it only on a set with a record of nothing but N: raw is 0 / 0 there)
        return "either"            # a non-finite distance ends the call: the pristine engine and finite_square() say which
    return None


def finite_square(measure, slot):
    """does every pair of the set have a finite distance (the oracle's)?  Small sets only."""
    import oracle
    d = oracle.all_pairs_square("n_high" if measure == "n" else measure, slot.codes, slot.base_counts(), threads=8)
    return bool(np.isfinite(d).all())


def _rows_of(op, got, model):
    """{row: the launch's values of that row, over its columns} for the picked rows of a pair run, with the geometry:
    (rows slot, cols slot, square, tallies, measure, {row: array})"""
    import distance_amd as da
    name = op[0]
    if name in ("run_square", "run_square_device"):
        m, rb, re = op[1], op[2], op[3]
        tallies = name == "run_square" and op[4]
        rs = cs = model.slot[0]
        rb, re = _window(rs.n, rb, re)
        base = da.square_row_start(rs.n, rb)
        out = {i: got[da.square_row_start(rs.n, i) - base:da.square_row_start(rs.n, i + 1) - base]
               for i in picked_rows(rs, rb, re, True)}
        return rs, cs, True, tallies, m, out
    if name == "run_slabs_square":
        m, tallies = op[1], op[5]
        rs = cs = model.slot[0]
        out = {i: got[da.square_row_start(rs.n, i):da.square_row_start(rs.n, i + 1)] for i in picked_rows(rs, 0, rs.n, True)}
        return rs, cs, True, tallies, m, out
    if name == "run_rect":
        m, rb, re, tallies = op[1], op[4], op[5], op[6]
        rs, cs = model.slot[op[2]], model.slot[op[3]]
        rb, re = _window(rs.n, rb, re)
        return rs, cs, False, tallies, m, {i: got[i - rb] for i in picked_rows(rs, rb, re, False)}
    if name == "run_slabs_rect":
        m, tallies = op[1], op[5]
        rs, cs = model.slot[op[2]], model.slot[op[3]]
        g = got.reshape((rs.n, cs.n) + got.shape[1:])
        return rs, cs, False, tallies, m, {i: g[i] for i in picked_rows(rs, 0, rs.n, False)}
    if name == "run_stream_batch":
        m, kind, nb, seed, tallies, counts = op[1:]
        cs = model.slot[0]
        rs = Slot(make_codes(kind, nb, cs.L, seed), caller_counts(nb, seed) if counts else None, -1)
        return rs, cs, False, tallies, m, {i: got[i] for i in picked_rows(rs, 0, rs.n, False)}
    if name == "stream":
        m, tallies, nibbles = op[1], op[7], op[8]
        cs = model.slot[0]
        codes, _, _ = _stream_batches(op, model)
        if nibbles:     # the 4-bit wire format keeps the high nibble: N, - and ? arrive as N (none of them is ever counted)
            codes = np.where((codes >> 4) == 15, np.uint8(240), codes)
        rs = Slot(codes, None, -2 - op[6])
        return rs, cs, False, tallies, m, {i: got[i] for i in picked_rows(rs, 0, rs.n, False)}
    return None


def check_against_the_oracle(op, got, model):
    """Source 1.  Returns the number of values held to the oracle."""
    import oracle
    import distance_amd as da
    name = op[0]
    if name == "base_counts":
        assert np.array_equal(got.astype(np.uint64), model.slot[op[1]].base_counts()), "base counts differ from the oracle's"
        return got.size
    if name == "consensus":
        sets = [model.slot[0].codes] + ([model.slot[1].codes] if op[1] and model.slot[1] is not None else [])
        assert np.array_equal(got, oracle.consensus(*sets)), "consensus differs from the oracle's"
        return got.size
    if name == "differences":
        s = model.slot[op[1]]
        cons = oracle.consensus(s.codes)
        lens, flat = got
        ends = np.cumsum(lens)
        for r in picked_rows(s, 0, s.n, False):
            mine = flat[ends[r] - lens[r]:ends[r]].astype(np.uint64)
            assert np.array_equal(mine, oracle.get_differences(s.codes[r], cons)), ("differences of record", r)
        return int(lens.sum())
    geo = _rows_of(op, got, model)
    if geo is None:
        return 0
    rs, cs, square, tallies, m, rows = geo
    if not rows:
        return 0
    om = "n_high" if m == "n" else m
    qc, tc = rs.base_counts(), cs.base_counts()
    f64 = ([], [], [], [], [])
    checked = 0
    for i, mine in rows.items():
        j0 = i + 1 if square else 0
        checked += len(mine)
        if tallies:
            want = model.oracle_tallies(m, rs, cs, i)[j0:] if rs.version > 0 else oracle.tallies_rect(
                "n_high" if m == "n" else "raw" if m == "jc69" else m, rs.codes[i:i + 1], cs.codes, threads=8)[0][j0:]
            assert np.array_equal(mine.astype(np.uint64), want), ("tallies of row", i, m)
            continue
        want = oracle.all_pairs_rect(om, rs.codes[i:i + 1], cs.codes[j0:], qc[i:i + 1], tc[j0:], threads=8)[0]
        if m in da.INT_MEASURES:
            assert np.array_equal(mine, want.astype(np.int64)), ("distances of row", i, m)
        elif m == "raw":      # one correctly rounded division: the reference's bits
            assert np.array_equal(mine.view(np.uint64), want.view(np.uint64)), ("distances of row", i, m)
        else:
            tl = (model.oracle_tallies(m, rs, cs, i) if rs.version > 0 else oracle.tallies_rect(
                "raw" if m == "jc69" else m, rs.codes[i:i + 1], cs.codes, threads=8)[0])[j0:]
            for lst, v in zip(f64, (mine, want, tl.astype(np.uint32), np.broadcast_to(qc[i], (len(mine), 4)), tc[j0:])):
                lst.append(v)
    if f64[0]:
        from test_gpu_launch_variants import check_f64
        import finalise_reference as fr
        g, w, tl, q, t = (np.concatenate(v) for v in f64)
        # check_f64 ties the oracle's value to the exact one within 2^-27 |x| before it uses either.  Where a logarithm's
        # argument 1 - e lies within 2^-20 of zero (saturated pairs: unrelated files, uniform codes) the f64 formula's own
        # rounding of 1 - e, 2^-53 / |1 - e| of it, passes that bar and decides between a huge value, inf and NaN: the exact
        # value says nothing about the reference there.  Those pairs are held to the oracle's own f64 value instead
        # (check_pole_pairs).
        with np.errstate(all="ignore"):
            pole = (np.abs(1 - fr.exact(m, tl, q, t).e) <= fr.LD(2.0 ** -20)).any(axis=1)
        keep = ~np.asarray(pole, bool)
        check_f64(m, np.ascontiguousarray(g[keep]), w[keep], tl[keep], q[keep], t[keep])
        check_pole_pairs(m, g[~keep], w[~keep])
    return checked


def check_pole_pairs(measure, got, want):
    """Pairs at a pole of the formula, against the oracle's f64 value: NaN, inf and zero where the oracle has them (the
    epilogue keeps the reference's operation order, so 1 - e rounds the same way), finite values within CLOSE_ULP of its
    bits — check_f64's own bar for every pair past the series switch, which these are."""
    if not len(got):
        return
    from test_gpu_finalise_accuracy import CLOSE_ULP
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    finite = np.isfinite(want) & (want != 0)
    ulp = np.abs(got[finite].view(np.int64) - want[finite].view(np.int64)) if finite.any() else np.zeros(0, np.int64)
    print("pole pairs of %s: %d (NaN %d, inf %d), largest distance from the oracle's bits %d ulp"
          % (measure, len(got), int(np.isnan(want).sum()), int(np.isinf(want).sum()), int(ulp.max()) if len(ulp) else 0))
    assert np.array_equal(np.isnan(got), np.isnan(want)), ("NaN pattern at the pole", measure)
    rest = ~finite & ~np.isnan(want)
    assert np.array_equal(got[rest].view(np.uint64), want[rest].view(np.uint64)), ("inf / zero at the pole", measure)
    assert np.isfinite(got[finite]).all() and (ulp <= CLOSE_ULP[measure]).all(), ("pole", measure, int(ulp.max()) if len(ulp) else 0)


# ------------------------------------------------------------------------------------------------ the second vocabulary
def _analysis_slots(op):
    """the slots an operation of the second vocabulary reads"""
    name = op[0]
    at = {"summary": 3, "group_summary": 5, "run_pairs": 3, "run_windows": 3, "nearest_windows": 4}.get(name)
    if at is not None:
        return (0,) if op[at] else (op[at + 1], op[at + 2])
    if name == "window_base_counts":
        return (op[1],)
    return (0,)


def _expected_error_analysis(op, model):
    name, s = op[0], model.slot
    if name in STREAM_OPS:
        return _expected_error_stream(op, model)
    slots = _analysis_slots(op)
    if any(s[k] is None for k in slots):
        return "either" if name.startswith("err_") else ERR_STATE      # (which refusal comes first is the library's order)
    if len(slots) == 2 and slots[0] == slots[1]:
        return ERR_ARG
    if len(slots) == 2 and model.widths_differ(*slots):
        return ERR_STATE
    if name == "err_capacity":
        return ERR_CAPACITY
    if name == "err_dendrogram_nonfinite":
        return ERR_STATE if s[0].n >= 2 else ERR_ARG   # (named only on a set with a record of nothing but N: raw is 0 / 0)
    if name.startswith("err_"):
        return ERR_ARG
    if name == "dendrogram":
        return ERR_ARG if s[0].n < 2 else "either"     # a non-finite distance ends the call, as for nj
    return None


def stream_is_stale(ms, model):
    """the documented refusal of a submit: a links stream when the loaded set's record count changed, a window-closest
    stream when its record count or its width did"""
    s0 = model.slot[0]
    if s0 is None:
        return True
    if ms.kind == "links":
        return s0.n != ms.n
    if ms.kind == "window_closest":
        return (s0.n, s0.L) != (ms.n, ms.L)
    return False


def _expected_error_stream(op, model):
    name, tag = op[0], op[1]
    if name == "stream_open":
        return ERR_STATE if model.slot[0] is None else None
    ms = model.streams[tag]
    keeps_lists = ms.kind in ("closest_loaded", "closest_streamed", "window_closest")
    if name in ("stream_push", "stream_push_bad"):
        if len(ms.in_flight) >= ms.depth:
            return ERR_STATE
        if stream_is_stale(ms, model) or (ms.poisoned and keeps_lists):
            return ERR_STATE
        return None
    if name == "stream_pop":
        if not ms.in_flight:
            return "either"
        return ERR_INVALID_CODE if ms.history[ms.in_flight[0]][3] else None
    if name == "stream_result":
        if ms.kind not in ("closest_loaded", "window_closest"):
            return ERR_ARG
        if ms.in_flight or ms.poisoned:
            return ERR_STATE
        if len(op) > 3 and op[3] is not None and op[3] < stream_entries(ms):
            return ERR_CAPACITY
        return None
    return None


def stream_records(ms):
    return sum(h[1] for h in ms.history if h[4])


def stream_entries(ms):
    """the entries of a closest or window-closest result so far: n_loaded [x n_windows] x min(k, records submitted)"""
    k = ms.op[4] if ms.kind == "closest_loaded" else ms.op[5]
    nw = len(window_list(ms.L, ms.op[4])) if ms.kind == "window_closest" else 1
    return ms.n * nw * min(k, stream_records(ms))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype.itemsize == 8 else a


def _canonical(n, i, j):
    i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
    return i * (2 * n - i - 1) // 2 + (j - i - 1)


ORACLE_PAIRS_MOST = 300 * 900      # the window lists' full payloads are asked of a pristine engine up to this many pairs


def check_analysis(op, got, model, payloads, window_payloads):
    """Source 1 for the second vocabulary: the reference module of each analysis, by the rule of that analysis's own GPU
    test module.  payloads(measure, square, rs, cs, tallies) is the whole result of run_square / run_rect on a pristine
    engine (what mst_reference, links_reference, summary_reference, group_summary_reference and representatives_reference
    are stated over; run_square and run_rect are themselves held to the oracle, above); window_payloads the same of
    run_windows.  The window calls and pair_sites are held to the oracle on the codes.  Returns the values compared."""
    import distance_amd as da
    name, s = op[0], model.slot
    if name == "mst":
        import mst_reference as mr
        _, m, _, tallies = op
        n = s[0].n
        want = mr.kruskal(n, payloads(m, True, 0, 0, False))
        assert np.array_equal(got[0].astype(np.int64), want[0]), ("mst edges", m)
        assert got[1].dtype == want[1].dtype and np.array_equal(_bits(got[1]), _bits(want[1])), ("mst values", m)
        if tallies:
            assert np.array_equal(got[3], payloads(m, True, 0, 0, True)[_canonical(n, want[0][:, 0], want[0][:, 1])]), ("mst tallies", m)
        return len(want[0])
    if name == "dendrogram":
        import dendrogram_reference as dr
        _, m, linkage, _ = op
        n = s[0].n
        dr.check_tree(got[0], got[1], got[2], n)
        want = dr.dendrogram(dr.square(n, payloads(m, True, 0, 0, False)), linkage)
        assert np.array_equal(got[0], want[0]), ("dendrogram parents", m, linkage)
        for g, w in zip(got[1:3], want[1:3]):
            assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), ("dendrogram lengths / heights", m, linkage)
        return 2 * n - 1
    if name in ("summary", "group_summary", "links"):
        at = {"summary": 3, "group_summary": 5, "links": 3}[name]
        m, square, rs, cs = op[1], op[at], op[at + 1], op[at + 2]
        rows, cols = (s[0], s[0]) if square else (s[rs], s[cs])
        vals = payloads(m, square, rs, cs, False).reshape(-1)
        if name == "summary":
            import summary_reference as sr
            thr, bins = op[2], op[7]
            sr.assert_summary(dict(got), sr.summary(m, vals, rows.n, cols.n, square, thr, bins=bins, width=summary_width(m)), op)
        elif name == "group_summary":
            import group_summary_reference as gr
            G, seed, thr = op[2], op[3], op[4]
            want = gr.group_summary(m, vals, rows.n, cols.n, square, thr, group_labels(rows.n, G, seed), G,
                                    None if square else group_labels(cols.n, 3, seed + 1), None if square else 3)
            gr.assert_group_summary(dict(got), want, op)
        else:
            import links_reference as lr
            thr, values, tallies = op[2], op[6], op[7]
            wi, wj, wv = lr.expected(m, vals, rows.n, cols.n, square, thr)
            assert np.array_equal(got[0], wi) and np.array_equal(got[1], wj), ("links", m, thr)
            if values:
                assert np.array_equal(_bits(got[2]), _bits(wv)), ("links values", m)
            if tallies:
                keep = lr.linked(m, vals, thr)
                assert np.array_equal(got[-1], payloads(m, square, rs, cs, True).reshape(len(vals), -1)[keep]), ("links tallies", m)
        return len(vals)
    if name == "representatives":
        import representatives_reference as rr
        _, m, thr, _, values, tallies = op
        n = s[0].n
        want = rr.reference(m, payloads(m, True, 0, 0, False), n, thr, payloads(m, True, 0, 0, True) if tallies else None)
        assert np.array_equal(got[0], want[0]), ("representatives", m, thr)
        if values:
            assert np.array_equal(_bits(got[1]), _bits(want[1])), ("representatives' values", m)
        if tallies:
            assert np.array_equal(got[-1], want[2]), ("representatives' tallies", m)
        return n
    if name == "run_pairs":        # bitwise what run_square / run_rect gives for each pair (the diagonal: the pristine engine's word)
        _, m, n_pairs, square, rs, cs, seed, values, tallies, _, _ = op
        rows, cols = (s[0], s[0]) if square else (s[rs], s[cs])
        row, col = (x.astype(np.int64) for x in pair_list(rows.n, cols.n, n_pairs, seed, square))
        off = row != col if square else np.ones(n_pairs, bool)
        pos = _canonical(rows.n, np.minimum(row, col), np.maximum(row, col))[off] if square else row * cols.n + col
        if values:
            assert np.array_equal(_bits(got[0][off]), _bits(payloads(m, square, rs, cs, False).reshape(-1)[pos])), ("run_pairs values", m)
        if tallies:
            full = payloads(m, square, rs, cs, True)
            assert np.array_equal(got[-1][off], full.reshape(-1, full.shape[-1])[pos]), ("run_pairs tallies", m)
        return int(off.sum())
    if name == "pair_sites":
        import pair_sites_reference as psr
        _, m, n_pairs, square, rs, cs, seed = op
        rows, cols = (s[0], s[0]) if square else (s[rs], s[cs])
        rng = np.random.default_rng([seed, 0x51735])
        row, col = rng.integers(0, rows.n, n_pairs), rng.integers(0, cols.n, n_pairs)
        for g, w in zip(got, psr.expected(m, rows.codes, cols.codes, row, col)):
            assert g.dtype == w.dtype and np.array_equal(g, w), ("pair_sites", m)
        return len(got[1])
    if name == "window_base_counts":
        import window_reference as wr
        sl = s[op[1]]
        assert np.array_equal(got, wr.expected_counts(sl.codes, window_list(sl.L, op[2]))), "window base counts"
        return got.size
    if name == "run_windows":
        import window_reference as wr
        import window_nearest_reference as wn
        _, m, which, square, rs, cs, rb, re, tallies = op
        rows, cols = (s[0], s[0]) if square else (s[rs], s[cs])
        windows = window_list(rows.L, which)
        rb, re = _window(rows.n, rb, re)
        last = min(re, rows.n - 1 if square else rows.n) - 1
        if last < rb:
            return 0
        checked = 0
        base = da.square_row_start(rows.n, rb) if square else 0
        for i in sorted({rb, last}):
            j0 = i + 1 if square else 0
            p0 = da.square_row_start(rows.n, i) - base if square else (i - rb) * cols.n
            mine = got[:, p0:p0 + cols.n - j0]
            tal = wr.expected_tallies(m, rows.codes[i:i + 1], cols.codes[j0:], windows)
            checked += mine.shape[0] * mine.shape[1]
            if tallies:
                assert np.array_equal(mine, tal), ("window tallies of row", i, m)
            elif m in ("n", "n_high", "raw"):
                want = wn.oracle_payloads(m, rows.codes[i:i + 1], cols.codes[j0:], windows)[:, 0, :]
                nan = np.isnan(want) if m == "raw" else np.zeros(want.shape, bool)      # (0 / 0 of an empty window: NaN of either sign)
                assert np.array_equal(nan, mine != mine) and np.array_equal(_bits(mine[~nan]), _bits(want[~nan])), ("window distances of row", i, m)
            else:           # the host's finalisation of the oracle's tallies (tn93: the counts inside the window), within 1e-12
                qc = wr.expected_counts(rows.codes[i:i + 1], windows)
                tc = wr.expected_counts(cols.codes[j0:], windows)
                for w in range(len(windows)):
                    for e in range(0, mine.shape[1], max(mine.shape[1] // 40, 1)):
                        f, v = da.finalize(m, tal[w, e], qc[w, 0], tc[w, e]), float(mine[w, e])
                        assert (f != f and v != v) or f == v or abs(f - v) <= 1e-12, ("window distance", i, w, e, m, f, v)
        return checked
    if name == "nearest_windows":
        import window_nearest_reference as wn
        _, m, which, k, square, rs, cs, tallies, _ = op
        rows, cols = (s[0], s[0]) if square else (s[rs], s[cs])
        if rows.n * cols.n > ORACLE_PAIRS_MOST:
            return 0
        lay = (lambda r: wn.full_square(r, rows.n)) if square else (lambda r: wn.full_rect(r, rows.n, cols.n))
        full = lay(window_payloads(m, which, square, rs, cs, False))
        index = wn.nearest(full, k, square)
        assert np.array_equal(got[0], index), ("nearest_windows index", m, which)
        assert np.array_equal(_bits(got[1]), _bits(wn.take(full, index))), ("nearest_windows values", m)
        if tallies:
            assert np.array_equal(got[2], wn.take(lay(window_payloads(m, which, square, rs, cs, True)), index)), ("nearest_windows tallies", m)
        return index.size
    return 0


ANALYSIS_ORACLE = ("mst", "dendrogram", "summary", "group_summary", "links", "representatives", "run_pairs", "pair_sites",
                   "window_base_counts", "run_windows", "nearest_windows")
ORACLE_ON_THE_CODES = ("pair_sites", "window_base_counts", "run_windows")      # the rest: references over the pristine engine's results


# ------------------------------------------------------------------------------------------------ the runner
class Runner:
    """One engine under test, its model, and the trace of what it was asked.  step() performs an operation, holds the
    answer to both sources and then lets the model follow.  At most two engines live at once: this one and the pristine
    one of the current check."""

    def __init__(self, analyses=False):
        import distance_amd as da
        self.da = da
        self.eng = da.Engine(0)
        self.model = Model()
        self.trace = []
        self.analyses = analyses    # hold the second vocabulary to its reference modules too (check_analysis)
        self.streams = {}           # the open dst_streams of the engine under test, by tag
        self._kept_payloads = {}    # the pristine engine's last whole result (_on_pristine)
        self.counts = {}            # operation name (a stream operation: "name kind") -> [pristine, oracle, reference] (_count)
        self.checked_ops = 0        # operations whose answer was held to the pristine engine (and the oracle where it speaks)
        self.state_ops = 0          # uploads, knobs, ids: nothing to compare, the model follows (shape and status asserted)
        self.checked_values = 0
        self.snapshot = None
        self.near_ties = 0
        self._streams = []          # the caller's streams: torch's, from its pool, alive as long as the Runner

    def close(self):
        for tag in list(self.streams):      # what a sequence left open
            self.streams.pop(tag).close()
        self.eng.close()

    def _count(self, key, source=0):
        """source 0: the pristine engine; 1: the CPU oracle on the model's bytes; 2: a reference module applied to the
        pristine engine's own whole results (not independent of the device code: those results are held to the oracle
        as run_square / run_rect / run_windows answers)"""
        c = self.counts.setdefault(key, [0, 0, 0])
        c[source] += 1

    def caller_stream(self, k=0):
        import torch
        while len(self._streams) <= k:
            self._streams.append(torch.cuda.Stream())
        return self._streams[k]

    def run(self, seq):
        for op in seq:
            self.step(op)
        return self

    def step(self, op):
        op = tuple(op)
        self.trace.append(op)
        try:
            self._step(op)
        except AssertionError as exc:
            raise AssertionError("%s\nafter: %s" % (exc, self._literal())) from None
        except Exception as exc:       # an unclean error is a finding too, and carries its sequence
            raise AssertionError("%s: %s\nafter: %s" % (type(exc).__name__, exc, self._literal())) from exc

    def _literal(self):
        return "replay(%r%s)" % (self.trace, ", analyses=True" if self.analyses else "")

    # -- introspection a directed sequence asserts
    def _state(self):
        e = self.eng
        return [e.run_records(0), e.run_records(1)] + [
            (e.planes_stored(k), e.set_info(k) if self.model.slot[k] is not None else None) for k in (0, 1)]

    def _check_op(self, op):
        e = self.eng
        if op[0] == "snapshot":
            self.snapshot = self._state()
            return
        what = op[1]
        if what == "unchanged":
            assert self._state() == self.snapshot, ("introspection moved", self.snapshot, self._state())
        elif what == "run_records":
            assert (e.run_records(op[2])[0] > 0) == op[3], ("run_records", op[2], e.run_records(op[2]))
        elif what == "planes_stored":
            assert e.planes_stored(op[2]) == op[3], ("planes_stored", op[2])
        elif what == "last_path":
            assert e.last_path() == op[2], ("last_path", e.last_path())
        elif what == "near_ties":      # the text call before this one sent values to the host's second look
            ties = e.text_stats()[0]
            assert ties > self.near_ties, "no near tie in the text: the host's base counts were not read"
            self.near_ties = ties
        else:
            raise ValueError(op)

    def _pristine(self, op):
        m = self.model
        with self.da.Engine(0) as p:
            p.set_path("dense")
            for k in (0, 1):
                if m.slot[k] is not None:
                    p.upload(k, m.slot[k].codes, m.slot[k].counts)
                if m.ids_ok(k):
                    p.set_ids(k, m.ids[k])
            return perform(p, op, m, self.caller_stream)

    def _on_pristine(self, key, call):
        """call(p) on a pristine engine that holds the model's slots, on the dense path; the last result is kept, under the
        uploads of the two slots and `key`"""
        m = self.model
        key = tuple(s.version if s is not None else 0 for s in m.slot) + key
        if key not in self._kept_payloads:
            with self.da.Engine(0) as p:
                p.set_path("dense")
                for k in (0, 1):
                    if m.slot[k] is not None:
                        p.upload(k, m.slot[k].codes, m.slot[k].counts)
                self._kept_payloads = {key: call(p)}      # one at a time: a whole result can be tens of megabytes
        return self._kept_payloads[key]

    def _payloads(self, measure, square, rs, cs, tallies):
        return self._on_pristine(("vals", measure, square, rs, cs, tallies), lambda p: (
            p.run_square(measure, tallies=tallies) if square else p.run_rect(measure, rs, cs, tallies=tallies)))

    def _window_payloads(self, measure, which, square, rs, cs, tallies):
        L = self.model.slot[0 if square else rs].L
        return self._on_pristine(("wvals", measure, which, square, rs, cs, tallies), lambda p: p.run_windows(
            measure, window_list(L, which), square=square, row_slot=rs, col_slot=cs, tallies=tallies))

    # -- open streams: a stream's answers depend on its own history and on slot 0, and on nothing else the context did
    def _replay_stream(self, ms, then=None):
        """On a pristine engine: slot 0, the same stream, the same batches with nothing in between, each collected at once.
        Returns (what every push answered, what every collect answered, then(engine, stream))."""
        m, da = self.model, self.da
        pushed, popped, extra = [], [], None
        with da.Engine(0) as p:
            p.set_path("dense")
            p.upload(0, m.slot[0].codes, m.slot[0].counts)
            st = open_stream(p, ms.op, ms.L)
            try:
                for kind, n, seed, bad, _ in ms.history:
                    try:
                        st.push(batch_codes(kind, n, ms.L, seed, bad))
                        pushed.append(None)
                    except da.DistanceError as exc:
                        pushed.append(("error", exc.status))
                        popped.append(None)
                        continue
                    try:
                        popped.append(_plain(st.pop()))
                    except da.DistanceError as exc:
                        popped.append(("error", exc.status))
                if then is not None:
                    try:
                        extra = then(p, st)
                    except da.DistanceError as exc:
                        extra = ("error", exc.status)
            finally:
                st.close()
        return pushed, popped, extra

    def _stream_definition(self, ms, got):
        """A closest stream on the loaded side and a window-closest stream, held to the header's definition on a pristine
        engine: the k smallest (key, ordinal) of the plain stream's own matrix of the same batches (closest_reference, as
        test_gpu_closest.py does), and dst_nearest_windows' rectangle form of slot 0 against the set of every record
        submitted so far.  Only for a history without a refused or invalid batch."""
        import closest_reference as cr
        m, da = self.model, self.da
        if any(h[3] or not h[4] for h in ms.history) or not ms.history:
            return 0
        nibbles, max_records = ms.op[-3], ms.op[-2]
        streamed = np.concatenate([batch_codes(h[0], h[1], ms.L, h[2]) for h in ms.history])
        with da.Engine(0) as p:
            p.set_path("dense")
            p.upload(0, m.slot[0].codes, m.slot[0].counts)
            if ms.kind == "closest_loaded":
                vals, tal = cr.plain_truth(p, ms.measure, streamed, max_records=max_records, nibbles=nibbles)
                want = cr.expected_for_loaded(vals, tal, ms.op[4])
            else:
                if nibbles:     # the 4-bit wire keeps the high nibble: N, - and ? arrive as N
                    streamed = np.where((streamed >> 4) == 15, np.uint8(240), streamed)
                p.upload(1, streamed)
                want = p.nearest_windows(ms.measure, window_list(ms.L, ms.op[4]), ms.op[5], square=False, row_slot=0, col_slot=1,
                                         tallies=True)
        for g, w, what in zip(got, want, ("index", "values", "tallies")):
            assert g.shape == w.shape and np.array_equal(_bits(g), _bits(w)), ("%s stream: %s differ from the definition" % (ms.kind, what))
        return got[0].size

    def _step_stream(self, op):
        name, tag, m = op[0], op[1], self.model
        want_err = expected_error(op, m)
        got = perform(self.eng, op, m, self.caller_stream, self.streams)
        failed = isinstance(got, tuple) and len(got) == 2 and got[0] == "error"
        if want_err is None:
            assert not failed, "%s failed with status %d: %s" % (name, got[1] if failed else 0, self.eng._lib.dst_last_error(self.eng._h).decode())
        elif want_err != "either":
            assert failed and got[1] == want_err, "%s: expected status %d, got %r" % (name, want_err, got if failed else "an answer")
        if name == "stream_open":
            if not failed:
                m.streams[tag] = ModelStream(op, m.slot[0])
            self.state_ops += 1
            return
        ms = m.streams[tag]
        key = "%s %s" % (name, ms.kind)
        stale = m.slot[0] is None or m.slot[0].version != ms.version      # (outside the contract: only the refusal is asserted)
        if name in ("stream_push", "stream_push_bad"):
            ms.history.append((op[2], op[3], op[4], name == "stream_push_bad", not failed))
            if not failed:
                ms.in_flight.append(len(ms.history) - 1)
                ms.popped = False
                self.state_ops += 1
            elif not stale:         # a refused submit: the pristine stream refuses it in the same way
                pushed, _, _ = self._replay_stream(ms)
                assert same(pushed[-1], got), "%s: a pristine stream with the same history answers %r" % (name, pushed[-1])
                self.checked_ops += 1
                self._count(key)
            else:
                ms.history.pop()
                self.checked_ops += 1
                self._count(key + " (slot 0 changed)")
        elif name == "stream_pop":
            at = ms.in_flight.pop(0) if ms.in_flight else None
            if at is not None and not stale:
                _, popped, _ = self._replay_stream(ms)
                assert same(got, popped[at]), "%s: batch %d differs from a pristine stream with the same history" % (key, at)
                self._count(key)
                if failed and ms.kind != "plain" and ms.kind != "links":
                    ms.poisoned = True
            ms.popped = True
            self.checked_ops += 1
        elif name == "stream_result":
            if not stale and not ms.in_flight:      # (with a batch in flight: the refusal, asserted above; the replay collects at once)
                args = (op[2], op[3] if len(op) > 3 else None)
                _, _, want = self._replay_stream(ms, lambda p, st: list(st.result(tallies=args[0], cap_entries=args[1])))
                assert same(got, want), "%s: differs from a pristine stream with the same history" % key
                self._count(key)
                if not failed and op[2]:
                    values = self._stream_definition(ms, got)
                    self.checked_values += values
                    if values:
                        self._count(key, 2)
            self.checked_ops += 1
        elif name == "stream_close":
            del m.streams[tag]
            self.state_ops += 1

    def _step(self, op):
        name = op[0]
        m = self.model
        if name in CHECKS:
            return self._check_op(op)
        if name in STREAM_OPS:
            return self._step_stream(op)
        want_err = expected_error(op, m)
        got = perform(self.eng, op, m, self.caller_stream)
        failed = isinstance(got, tuple) and len(got) == 2 and got[0] == "error"
        if want_err is None:
            assert not failed, ("%s failed with status %d: %s" % (name, got[1], self.eng._lib.dst_last_error(self.eng._h).decode())
                                if failed else "")
        elif want_err != "either":
            assert failed and got[1] == want_err, ("%s: expected status %d, got %r" % (name, want_err, got if failed else "an answer"))
        cls = op_class(op)
        if cls not in ("upload", "knob") and name not in ("set_ids", "bad_upload"):
            want = self._pristine(op)
            assert same(got, want), "%s: differs from a pristine engine's answer on the dense path" % name
            if not failed:
                if name in ("nj", "nj_bootstrap") and m.slot[0].n <= 300:
                    assert finite_square(op[1], m.slot[0]), "nj answered although the oracle has a non-finite distance"
                values = check_against_the_oracle(op, got, m)
                self.checked_values += values
                if values:
                    self._count(name, 1)
                self._check_last_path(op)
                if name == "dendrogram" and m.slot[0].n <= 300:
                    assert finite_square(op[1], m.slot[0]), "dendrogram answered although the oracle has a non-finite distance"
                if self.analyses and name in ANALYSIS_ORACLE:
                    values = check_analysis(op, got, m, self._payloads, self._window_payloads)
                    self.checked_values += values
                    if values:
                        self._count(name, 1 if name in ORACLE_ON_THE_CODES else 2)
            elif name in ("nj", "nj_bootstrap") and m.slot[0] is not None and 3 <= m.slot[0].n <= 300:
                assert not finite_square(op[1], m.slot[0]), "nj failed although every distance is finite"
            elif name == "dendrogram" and m.slot[0] is not None and 2 <= m.slot[0].n <= 300:
                assert not finite_square(op[1], m.slot[0]), "dendrogram failed although every distance is finite"
            self.checked_ops += 1
            self._count(name)
        else:
            self.state_ops += 1
        self._commit(op)

    def _check_last_path(self, op):
        """where the model can tell: a forced dense path, and a forced consensus path on a shape the lists can index"""
        if op_class(op) not in ("square", "rect") or op[0].startswith("run_slabs"):
            return
        m = self.model
        rows = m.slot[op[2]] if op[0] == "run_rect" else m.slot[0]
        cols = m.slot[op[3]] if op[0] == "run_rect" else m.slot[0]
        rb, re = (op[4], op[5]) if op[0] == "run_rect" else (op[2], op[3])
        rb, re = _window(rows.n, rb, re)
        pairs = (re - rb) * cols.n if op[0] == "run_rect" else self.da.square_row_start(rows.n, re) - self.da.square_row_start(rows.n, rb)
        if pairs == 0:
            return
        if m.path == "dense":
            assert self.eng.last_path() == "dense", self.eng.last_path()
        elif m.path == "consensus":
            assert self.eng.last_path() == "consensus", self.eng.last_path()

    def _commit(self, op):
        name, m = op[0], self.model
        if name in ("upload", "upload_device"):
            _, slot, kind, n, L, seed, flag = op
            m.set_slot(slot, make_codes(kind, n, L, seed), caller_counts(n, seed) if name == "upload" and flag else None)
            assert self.eng.set_info(slot) == (n, L)
            if m.path == "dense" or m.prep == "huge":      # no fused preparation: every plane stored, no run records
                assert self.eng.planes_stored(slot) and self.eng.run_records(slot) == (0, 0)
        elif name == "bad_upload":
            m.slot[op[1]] = None
            assert not self.eng.planes_stored(op[1])
        elif name == "run_stream_batch":
            _, _, kind, nb, seed, _, counts = op
            # Engine.run_stream_batch uploads the batch to slot 1 and then runs: whether or not the run failed (slot 0 not
            # loaded: the batch is 100 sites wide then), slot 1 holds the batch — asked of the engine, not assumed
            L = m.slot[0].L if m.slot[0] is not None else 100
            assert self.eng.set_info(1) == (nb, L), ("slot 1 after a streamed batch", self.eng.set_info(1))
            m.set_slot(1, make_codes(kind, nb, L, seed), caller_counts(nb, seed) if counts else None)
        elif name == "set_ids":
            n = m.slot[op[1]].n if m.slot[op[1]] is not None else 3
            m.ids[op[1]] = id_list(op[2], n)
        elif name == "set_path":
            m.path = op[1]
        elif name == "set_prep":
            m.prep = op[1]
        elif name == "set_variant":
            m.variant = op[1]
        elif name == "set_ksplit":
            m.ksplit = op[1]


def replay(seq, analyses=False, counts=None):
    """Run a sequence (the literal a failure printed) on a fresh engine; returns (operations whose answer was compared,
    state operations the model followed, values held to the oracle).  analyses: the second vocabulary's reference modules
    too; counts: a dict that receives, per operation name, how often it was held to the pristine engine, to the CPU oracle on
    the bytes, and to a reference module over the pristine engine's whole results (Runner._count)."""
    r = Runner(analyses)
    try:
        r.run(seq)
        if counts is not None:
            for key, got in r.counts.items():
                c = counts.setdefault(key, [0, 0, 0])
                for k in range(3):
                    c[k] += got[k]
        return r.checked_ops, r.state_ops, r.checked_values
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------ the seeded walk
WALK_N = (1, 2, 65, 300, 900, 2500)
WALK_L = (1, 127, 129, 1000, 4100, 6000)
CLASS_WEIGHT = {"upload": 2.0, "knob": 2.0, "square": 3.0, "rect": 2.0, "stream": 1.5, "text": 1.5, "derived": 1.5, "error": 1.0}


def _kinds_for(n, L):
    kinds = ["low", "diverse", "uniform"]
    if L >= 1000 and n >= 65:
        kinds.append("clade")           # hot columns need sites to be 2 % of
    if L >= 4100 and 65 <= n <= 900:
        kinds += ["runs", "clade_runs"]  # four whole chunks of N need a run of 640 sites
    return kinds


def _rows(rng, n, most=96):
    """a row range: everything for small sets, else a window of at most `most` rows at the start, the end or between"""
    if n <= most and rng.random() < 0.6:
        return 0, n
    w = int(rng.integers(1, min(most, n) + 1))
    where = rng.integers(0, 3)
    rb = 0 if where == 0 else n - w if where == 1 else int(rng.integers(0, n - w + 1))
    return rb, rb + w


def walk(seed):
    """25-40 operations drawn from the vocabulary.  After an operation that changes state (upload, knob) the pair runs weigh
    three times as much; a pair of consecutive classes not yet seen in this walk weighs four times as much, so that a few
    seeds cover every ordered pair of CLASSES.  Deterministic in `seed`."""
    rng = np.random.default_rng([seed, 0x5E9])
    length = int(rng.integers(25, 41))
    shape = [None, None]      # (kind, n, L) of each slot as the walk knows it
    ids = [0, 0]              # the record count the slot's ids were given for
    seen = set()
    L0 = int(rng.choice(WALK_L))
    n0 = int(rng.choice(WALK_N[2:]))
    ops = [("upload", 0, str(rng.choice(_kinds_for(n0, L0))), n0, L0, int(rng.integers(1, 10_000)), False)]
    shape[0] = (ops[0][2], n0, L0)
    prev = "upload"
    m_of = lambda: str(rng.choice(ALL))   # noqa: E731

    def upload(slot):
        other = shape[1 - slot]
        L = other[2] if other is not None and rng.random() < 0.75 else int(rng.choice(WALK_L))
        n = int(rng.choice(WALK_N if slot == 0 else WALK_N[:5]))
        kind = str(rng.choice(_kinds_for(n, L)))
        shape[slot] = (kind, n, L)
        seed_u = int(rng.integers(1, 10_000))
        if rng.random() < 0.3:
            return ("upload_device", slot, kind, n, L, seed_u, bool(rng.random() < 0.5))
        return ("upload", slot, kind, n, L, seed_u, bool(rng.random() < 0.3))

    def draw(cls):
        n = shape[0][1] if shape[0] is not None else 3
        both = shape[0] is not None and shape[1] is not None
        if cls == "upload":
            return upload(int(rng.integers(0, 2)))
        if cls == "knob":
            k = rng.integers(0, 6)
            if k < 3:
                return ("set_path", str(rng.choice(PATH_NAMES)))
            if k == 3:
                return ("set_prep", str(rng.choice(list(PREP))))
            if k == 4:
                return ("set_variant", int(rng.integers(0, 3)))
            return ("set_ksplit", int(rng.choice([0, 1, 3])))
        if cls == "square":
            rb, re = _rows(rng, n)
            k = rng.integers(0, 8)
            if k == 0 and n <= 300:
                return ("run_slabs_square", m_of(), 0, 0, int(rng.choice([1000, 20_000])), bool(rng.random() < 0.5))
            if k == 1:
                return ("run_square_device", m_of(), rb, re)
            return ("run_square", m_of(), rb, re, bool(rng.random() < 0.4))
        if cls == "rect":
            rs = int(rng.integers(0, 2))
            nr = shape[rs][1] if shape[rs] is not None else 3
            rb, re = _rows(rng, nr)
            if rng.random() < 0.15 and both and shape[0][1] * shape[1][1] <= 300 * 900:
                return ("run_slabs_rect", m_of(), rs, 1 - rs, int(rng.choice([5000, 50_000])), bool(rng.random() < 0.5))
            return ("run_rect", m_of(), rs, 1 - rs, rb, re, bool(rng.random() < 0.4))
        if cls == "stream":
            kind = str(rng.choice(["low", "diverse"]))
            if rng.random() < 0.5:
                L = shape[0][2] if shape[0] is not None else 100
                nb = int(rng.choice([1, 7, 40]))
                shape[1] = (kind, nb, L)
                return ("run_stream_batch", m_of(), kind, nb, int(rng.integers(1, 10_000)), bool(rng.random() < 0.4), bool(rng.random() < 0.3))
            return ("stream", m_of(), kind, int(rng.choice([5, 19])), int(rng.choice([4, 8])), int(rng.choice([2, 3])),
                    int(rng.integers(1, 10_000)), bool(rng.random() < 0.4), bool(rng.random() < 0.5))
        if cls == "text":
            k = rng.integers(0, 5)
            if k == 0 or not ids[0]:
                slot = 0 if not ids[0] else int(rng.integers(0, 2))
                ids[slot] = shape[slot][1] if shape[slot] is not None else 3
                return ("set_ids", slot, "id%d_" % int(rng.integers(0, 100)))
            rb, re = _rows(rng, n, most=6)
            if k == 1 or k == 4:
                return ("text_square", m_of(), rb, re)
            if k == 2:
                rs = int(rng.integers(0, 2))
                rb, re = _rows(rng, shape[rs][1] if shape[rs] is not None else 3, most=6)
                return ("text_rect", m_of(), rs, 1 - rs, rb, re, bool(rng.random() < 0.5))
            return ("text_matrix", m_of(), True, 0, 1, rb, re, str(rng.choice(["tsv", "phylip"])))
        if cls == "derived":
            k = rng.integers(0, 8)
            if k == 0:
                return ("nearest", m_of(), int(rng.choice([1, 5])), True, 0, 1)
            if k == 1:
                rs = int(rng.integers(0, 2))
                return ("nearest", m_of(), int(rng.choice([1, 5])), False, rs, 1 - rs)
            if k == 2:
                return ("clusters", m_of(), float(rng.choice([0.0, 0.004, 3.0])))
            if k == 3 and n <= 300:
                return ("nj", m_of())
            if k == 4 and n <= 300:
                return ("nj_bootstrap", m_of(), 3, int(rng.integers(1, 100)))
            if k == 5:
                return ("consensus", bool(rng.random() < 0.5))
            if k == 6:
                return ("differences", int(rng.integers(0, 2)))
            return ("base_counts", int(rng.integers(0, 2)))
        k = rng.integers(0, 5)        # error
        if k == 0:
            slot = int(rng.integers(0, 2))
            shape[slot] = None
            return ("bad_upload", slot, int(rng.choice([2, 65, 300])), int(rng.choice([129, 1000])), int(rng.integers(1, 10_000)))
        if k == 1:
            return ("err_text_capacity", m_of())
        if k == 2 and shape[0] is not None and shape[0][0] in ("runs", "clade_runs"):
            return ("err_nj_nonfinite", "raw")
        if k == 3 and n <= 300:
            return ("clusters_tiny_slabs", m_of(), float(rng.choice([0.004, 3.0])))
        return ("err_width", 0)

    ops.append(upload(1))
    while len(ops) < length:
        w = np.array([CLASS_WEIGHT[c] * (3.0 if prev in ("upload", "knob") and c in ("square", "rect", "stream") else 1.0)
                      * (4.0 if (prev, c) not in seen else 1.0) for c in CLASSES])
        cls = str(rng.choice(CLASSES, p=w / w.sum()))
        if shape[0] is None and cls not in ("upload", "error", "knob"):      # a rejected upload of slot 0: one use of it, then a new set
            if prev == "error" and ops[-1][0] == "bad_upload":
                cls = str(rng.choice(["square", "derived"]))
            else:
                cls = "upload"
        op = upload(0) if cls == "upload" and shape[0] is None else draw(cls)
        ops.append(op)
        seen.add((prev, cls))
        prev = cls
    return ops


# ------------------------------------------------------------------------------------------------ the second seeded walk
AWALK_N = (2, 65, 300, 900)
AWALK_L = (127, 129, 1000, 4100)
AWALK_BATCH = (1, 7, 40)
ACLASS_WEIGHT = {"upload": 1.5, "knob": 2.0, "pair": 2.0, "slab": 3.0, "window": 2.5, "pairlist": 2.0, "handle": 4.5, "error": 1.0}
KEEPS_LISTS = ("closest_loaded", "closest_streamed", "window_closest")


def walk_analyses(seed):
    """25-40 operations drawn from the second vocabulary, built like walk(): weights per class, three times as much for a
    call that computes after an upload or a knob, four times as much for a pair of consecutive classes this walk has not
    seen.  Streams are handles: a walk opens at most two, pushes batches of 1, 7 and 40 records, collects, asks for the
    lists and closes, with whatever else it draws in between; what is open at the end the runner closes.  While a
    stream is open slot 0 is not uploaded to (the header: it stays loaded and unchanged).  Deterministic in `seed`."""
    rng = np.random.default_rng([seed, 0xA7A1])
    length = int(rng.integers(25, 41))
    shape = [None, None]
    seen = set()
    streams = {}          # tag -> {"kind", "depth", "flying": [bad, ...], "pushes", "poisoned"}
    tags = iter("abcdefghijklmnopqrstuvwxyz")
    m_of = lambda: str(rng.choice(ALL))   # noqa: E731
    flag = lambda p=0.5: bool(rng.random() < p)   # noqa: E731
    thr_of = lambda: float(rng.choice([0.0, 0.004, 3.0]))   # noqa: E731

    def upload(slot):
        other = shape[1 - slot]
        L = other[2] if other is not None and rng.random() < 0.75 else int(rng.choice(AWALK_L))
        n = int(rng.choice(AWALK_N))
        kind = str(rng.choice(_kinds_for(n, L)))
        shape[slot] = (kind, n, L)
        seed_u = int(rng.integers(1, 10_000))
        if rng.random() < 0.25:
            return ("upload_device", slot, kind, n, L, seed_u, flag())
        return ("upload", slot, kind, n, L, seed_u, flag(0.3))

    def max_pairs():
        return int(rng.choice([0, 500, 20_000] if shape[0][1] <= 300 else [0, 20_000]))

    def sides():
        """(square, row slot, col slot): the rectangle in both orders"""
        if flag(0.55):
            return True, 0, 1
        rs = int(rng.integers(0, 2))
        return False, rs, 1 - rs

    def outputs():
        """(values, tallies) of run_pairs: one of them at least"""
        values, tallies = flag(0.8), flag(0.4)
        return (values or not tallies, tallies)

    def handle():
        usable = [t for t, s in streams.items()]
        if not usable or (len(usable) < 2 and rng.random() < 0.3):
            tag, kind, m = next(tags), str(rng.choice(STREAM_KINDS)), m_of()
            depth = int(rng.choice([2, 3]))
            tail = (flag(), 40, depth)
            if kind == "plain":
                args = (flag(0.4),)
            elif kind in ("closest_loaded", "closest_streamed"):
                args = (int(rng.choice([1, 5])),)
            elif kind == "links":
                args = (float(rng.choice([0.004, 3.0])), flag(0.7), flag(0.4), int(rng.choice([0, 1000])))
            else:
                args = (str(rng.choice(["all", "other", "few"])), int(rng.choice([1, 3])), int(rng.choice([0, 50_000])))
            streams[tag] = {"kind": kind, "depth": depth, "flying": [], "pushes": 0, "poisoned": False}
            return ("stream_open", tag, kind, m) + args + tail
        tag = str(rng.choice(usable))
        s = streams[tag]
        if s["poisoned"]:
            del streams[tag]
            return ("stream_close", tag)
        if len(s["flying"]) == s["depth"] - 1:
            return pop(tag)
        k = rng.random()
        if k < 0.5:
            return push(tag, False)
        if k < 0.75 and s["flying"]:
            return pop(tag)
        if k < 0.9 and s["kind"] in ("closest_loaded", "window_closest") and not s["flying"] and s["pushes"]:
            return ("stream_result", tag, flag(0.7))
        if k >= 0.9 and not s["flying"] and s["pushes"]:
            del streams[tag]
            return ("stream_close", tag)
        return push(tag, False)

    def push(tag, bad):
        s = streams[tag]
        s["flying"].append(bad)
        s["pushes"] += 1
        return ("stream_push_bad" if bad else "stream_push", tag, str(rng.choice(["low", "diverse"])), int(rng.choice(AWALK_BATCH)),
                int(rng.integers(1, 10_000)))

    def pop(tag):
        s = streams[tag]
        if s["flying"].pop(0) and s["kind"] in KEEPS_LISTS:
            s["poisoned"] = True
        return ("stream_pop", tag)

    def draw(cls):
        n = shape[0][1]
        if cls == "upload":
            return upload(1 if streams else int(rng.integers(0, 2)))
        if cls == "knob":
            k = rng.integers(0, 6)
            if k < 3:
                return ("set_path", str(rng.choice(PATH_NAMES)))
            if k == 3:
                return ("set_prep", str(rng.choice(list(PREP))))
            if k == 4:
                return ("set_variant", int(rng.integers(0, 3)))
            return ("set_ksplit", int(rng.choice([0, 1, 3])))
        if cls == "pair":
            if flag(0.6):
                rb, re = _rows(rng, n)
                return ("run_square", m_of(), rb, re, flag(0.4))
            rs = int(rng.integers(0, 2))
            rb, re = _rows(rng, shape[rs][1])
            return ("run_rect", m_of(), rs, 1 - rs, rb, re, flag(0.4))
        if cls == "slab":
            k = rng.integers(0, 8)
            if k == 0:
                return ("mst", m_of(), max_pairs(), flag())
            if k == 1 and n <= 300:
                return ("dendrogram", str(rng.choice(["n", "n_high", "k80", "tn93"])), str(rng.choice(LINKAGES)), max_pairs())
            if k == 2:
                return ("summary", m_of(), thr_of()) + sides() + (max_pairs(), int(rng.choice([0, 16])))
            if k == 3:
                return ("group_summary", m_of(), int(rng.choice([1, 4])), int(rng.integers(1, 100)), thr_of()) + sides() + (max_pairs(),)
            if k == 4:
                return ("representatives", m_of(), thr_of(), max_pairs(), flag(0.7), flag(0.4))
            if k == 5:
                return ("nearest", m_of(), int(rng.choice([1, 5]))) + sides()
            return ("links", m_of(), float(rng.choice([0.0, 0.004]))) + sides() + (flag(0.7), flag(0.4), max_pairs())
        if cls == "window":
            k = rng.integers(0, 5)
            which = str(rng.choice(["all", "other", "few"]))
            if k < 2:
                square, rs, cs = sides()
                rb, re = _rows(rng, shape[0 if square else rs][1])
                return ("run_windows", m_of(), which, square, rs, cs, rb, re, flag())
            if k == 2:
                return ("window_base_counts", int(rng.integers(0, 2)), which)
            return ("nearest_windows", m_of(), which, int(rng.choice([1, 2, 5]))) + sides() + (flag(0.4), int(rng.choice([0, 200_000])))
        if cls == "pairlist":
            if flag(0.7):
                return (("run_pairs", m_of(), int(rng.choice([3, 64, 5000]))) + sides() +
                        (int(rng.integers(1, 100)),) + outputs() + (max_pairs(), str(rng.choice(["auto", "direct", "sweep"]))))
            return ("pair_sites", m_of(), 64) + sides() + (int(rng.integers(1, 100)),)
        if cls == "handle":
            return handle()
        k = rng.integers(0, 8)        # error
        ready = [t for t, s in streams.items() if not s["poisoned"] and len(s["flying"]) < s["depth"] - 1]
        if k < 2 and ready:
            return push(str(rng.choice(ready)), True)
        if k == 2:
            return ("err_pairs_index", m_of())
        if k == 3:
            return ("err_window", str(rng.choice(["reversed", "past"])))
        if k == 4:
            return ("err_label", m_of())
        if k == 5:
            return ("err_k", m_of(), int(rng.choice([0, 257])))
        if k == 6 and shape[0][0] in ("runs", "clade_runs") and n <= 300:
            return ("err_dendrogram_nonfinite", "raw")
        return ("err_capacity", m_of())

    ops = [upload(0), upload(1)]
    if rng.random() < 0.5:      # half the walks start prepared for the lists: run records, deferred planes
        ops = [("set_prep", "zero")] + ops
    prev = "upload"
    computing = ("pair", "slab", "window", "pairlist", "handle")
    while len(ops) < length:
        w = np.array([ACLASS_WEIGHT[c] * (3.0 if prev in ("upload", "knob") and c in computing else 1.0)
                      * (4.0 if (prev, c) not in seen else 1.0) for c in ANALYSIS_CLASSES])
        cls = str(rng.choice(ANALYSIS_CLASSES, p=w / w.sum()))
        op = draw(cls)
        cls = ANALYSIS_OPS[op[0]]
        ops.append(op)
        seen.add((prev, cls))
        prev = cls
    return ops
