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


def op_class(op):
    return OP_CLASS.get(op[0]) or DIRECTED_OPS.get(op[0])


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


def perform(eng, op, model, caller_stream=None):
    """Run `op` on `eng`; the result as plain data, or ("error", status).  Uploads and knobs return None.
    caller_stream: the Runner's streams, by number (Runner.caller_stream)."""
    import distance_amd as da
    try:
        return _perform(eng, op, model, caller_stream)
    except da.DistanceError as exc:
        return ("error", exc.status)


def _perform(eng, op, model, caller_stream):
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
        _, m, thr, square, rs, cs, values, tallies = op
        return list(eng.links(m, thr, square=square, row_slot=rs, col_slot=cs, values=values, tallies=tallies))
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


# ------------------------------------------------------------------------------------------------ the runner
class Runner:
    """One engine under test, its model, and the trace of what it was asked.  step() performs an operation, holds the
    answer to both sources and then lets the model follow.  At most two engines live at once: this one and the pristine
    one of the current check."""

    def __init__(self):
        import distance_amd as da
        self.da = da
        self.eng = da.Engine(0)
        self.model = Model()
        self.trace = []
        self.checked_ops = 0        # operations whose answer was held to the pristine engine (and the oracle where it speaks)
        self.state_ops = 0          # uploads, knobs, ids: nothing to compare, the model follows (shape and status asserted)
        self.checked_values = 0
        self.snapshot = None
        self.near_ties = 0
        self._streams = []          # the caller's streams: torch's, from its pool, alive as long as the Runner

    def close(self):
        self.eng.close()

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
            raise AssertionError("%s\nafter: replay(%r)" % (exc, self.trace)) from None
        except Exception as exc:       # an unclean error is a finding too, and carries its sequence
            raise AssertionError("%s: %s\nafter: replay(%r)" % (type(exc).__name__, exc, self.trace)) from exc

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

    def _step(self, op):
        name = op[0]
        m = self.model
        if name in CHECKS:
            return self._check_op(op)
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
                self.checked_values += check_against_the_oracle(op, got, m)
                self._check_last_path(op)
            elif name in ("nj", "nj_bootstrap") and m.slot[0] is not None and 3 <= m.slot[0].n <= 300:
                assert not finite_square(op[1], m.slot[0]), "nj failed although every distance is finite"
            self.checked_ops += 1
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


def replay(seq):
    """Run a sequence (the literal a failure printed) on a fresh engine; returns (operations whose answer was compared,
    state operations the model followed, values held to the oracle)."""
    r = Runner()
    try:
        r.run(seq)
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
