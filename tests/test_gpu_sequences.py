"""The answer does not depend on what the context did before: sequences of operations on ONE engine.

Every other module uploads and then makes one kind of call.  Here an engine lives through a sequence — uploads of both
slots in every kind and shape, knob changes, square, rectangle, stream and slab runs, text, nearest, clusters, NJ,
bootstrap, accessors and errors — and EVERY operation of it is held to the oracle and to a pristine engine on the dense
path (tests/engine_model.py).  DIRECTED names the orders the cache keys of DeviceSet / dst_ctx imply; SEEDS are random
walks over the whole vocabulary.  A failure prints the sequence up to the failing operation as a replay([...]) literal.

Without a GPU: the walk generator is deterministic, and the committed seeds with the directed sequences reach every
operation and every ordered pair of consecutive operation classes (engine_model.CLASSES).
"""
import numpy as np
import pytest

import engine_model as em
from engine_model import replay   # noqa: F401  (what a failure's message names)

gpu = pytest.mark.gpu
ALL = em.ALL
WALK = ("n", "tn93", "raw", "k80", "n_high", "jc69")      # a family walk: 0, 3, 1, 2, 0, 1 (aconst_family, corr_family)


def both_outputs(measures, rb, re, rb2, re2):
    """distances of one row window and tallies of another, measure after measure"""
    ops = []
    for m in measures:
        ops += [("run_square", m, rb, re, False), ("run_square", m, rb2, re2, True)]
    return ops


def advice_order(path):
    """ADVICE.md's order: a stripped set as the ROW set of a rectangle, then a square run (ensure_index must not take the
    pack's stripped counts for the lists it just built whole), then as the column set, then a square run again"""
    kind = "clade_runs" if path == "hybrid" else "runs"
    return [("set_prep", "zero"), ("upload", 0, kind, 600, 4100, 11, False), ("upload", 1, "low", 130, 4100, 12, False),
            ("set_path", path), ("expect", "run_records", 0, True),
            ("run_rect", "k80", 0, 1, 0, 600, False), ("run_square", "k80", 0, 96, False), ("run_square", "tn93", 504, 600, True),
            ("expect", "last_path", path),
            ("run_rect", "tn93", 1, 0, 0, 130, False), ("expect", "run_records", 0, False),
            ("run_square", "raw", 0, 96, False), ("run_square", "k80", 300, 364, True), ("run_square", "n", 590, 600, False),
            ("expect", "last_path", path)]


def path_walk():
    """one upload of a stripped set with hot columns, every path in turn (rec.without_hot, pre_cold / pre_hot, runs.known,
    the correction tables with and without the hot sites)"""
    ops = [("set_prep", "zero"), ("upload", 0, "clade_runs", 600, 4100, 21, False), ("expect", "run_records", 0, True)]
    for path in ("consensus", "hybrid", "consensus", "dense", "auto", "hybrid"):
        ops += [("set_path", path), ("run_square", "k80", 0, 64, False), ("run_square", "tn93", 536, 600, True),
                ("run_square", "raw", 250, 314, False)]
        if path != "auto":
            ops.append(("expect", "last_path", path))
    return ops


def family_walk():
    """measure families back and forth on one set and between two (no run records here: low diversity only)"""
    ops = [("set_prep", "zero"), ("upload", 0, "low", 700, 3000, 31, False), ("upload", 1, "low", 90, 3000, 32, True),
           ("set_path", "consensus"), ("expect", "run_records", 0, False)]
    ops += both_outputs(WALK + WALK[::-1], 0, 64, 600, 700)
    for m in WALK + WALK[::-1]:
        ops += [("run_rect", m, 1, 0, 0, 90, m in ("raw", "tn93")), ("run_rect", m, 0, 1, 630, 700, m in ("k80", "n"))]
    ops.append(("expect", "last_path", "consensus"))
    return ops


def reference_ownership(path):
    """whose reference the lists, the constants and the hot columns were made against (ref_owner, ref_epoch, hot_ref_*,
    aconst_ref_*): both directions, then each slot re-uploaded alone"""
    kind = "clade" if path == "hybrid" else "low"
    r01 = [("run_rect", "k80", 0, 1, 0, 500, False), ("run_rect", "tn93", 0, 1, 400, 500, True)]
    r10 = [("run_rect", "k80", 1, 0, 0, 200, False), ("run_rect", "raw", 1, 0, 100, 200, True)]
    return ([("set_prep", "zero"), ("upload", 0, kind, 500, 3000, 41, False), ("upload", 1, kind, 200, 3000, 42, False),
             ("set_path", path)] + r01 + r10 + r01 + [("upload", 1, kind, 200, 3000, 43, False)] + r01 +
            [("upload", 0, kind, 500, 3000, 44, False)] + r10 + r01 + [("expect", "last_path", path)])


def same_shape_new_content():
    """the epoch is all that tells two uploads of one shape apart (text_counts_epoch, aconst_epoch, hot_epoch, pre_epoch);
    then a smaller shape in buffers that keep their size, and every reader"""
    ops = [("set_prep", "zero"), ("set_path", "consensus")]
    for seed in (51, 52, 53):
        ops += [("upload", 0, "low", 900, 3000, seed, False), ("set_ids", 0, "s%d_" % seed), ("run_square", "tn93", 0, 64, False),
                ("text_square", "tn93", 0, 160), ("expect", "near_ties"), ("run_square", "k80", 800, 900, True),
                ("text_matrix", "tn93", True, 0, 1, 0, 8, "tsv"), ("nearest", "tn93", 3, True, 0, 1)]
    ops += [("upload", 0, "clade", 300, 1000, 54, False), ("upload", 1, "low", 65, 1000, 55, False), ("set_ids", 0, "t"),
            ("set_ids", 1, "u"), ("run_square", "tn93", 0, 300, False), ("run_square", "raw", 0, 300, True),
            ("text_square", "tn93", 0, 40), ("text_rect", "k80", 1, 0, 0, 65, True), ("text_matrix", "jc69", False, 0, 1, 0, 20, "phylip"),
            ("nearest", "k80", 5, True, 0, 1), ("nearest", "raw", 2, False, 1, 0), ("clusters", "n_high", 3.0), ("nj", "n_high"),
            ("nj_bootstrap", "n_high", 3, 7), ("base_counts", 0), ("consensus", True), ("differences", 0),
            ("run_slabs_square", "tn93", 0, 0, 9000, False), ("run_slabs_rect", "k80", 1, 0, 5000, True),
            ("run_stream_batch", "tn93", "low", 20, 56, False, True), ("stream", "raw", "low", 19, 8, 3, 57, False, True)]
    return ops


def wide_narrow_wide():
    """L = 70,000 (32-bit accumulators, 18 mask words, DST_OUT_TALLY hot tallies), then 4,000, then 70,000 again in the
    same context (aconst_wide, the hot tallies' kind, the run masks' words)"""
    ops = [("set_prep", "zero")]
    for kind, L, seed in (("wide", 70_000, 61), ("clade", 4_000, 62), ("wide_clade", 70_000, 63)):
        ops += [("set_path", "auto"), ("upload", 0, kind, 160, L, seed, False), ("set_path", "consensus"),
                ("run_square", "k80", 0, 160, False), ("run_square", "tn93", 0, 160, True), ("expect", "last_path", "consensus"),
                ("set_path", "hybrid"), ("run_square", "tn93", 0, 160, False), ("run_square", "raw", 96, 160, True),
                ("set_path", "dense"), ("run_square", "n", 0, 160, False)]
    return ops


def deferred_planes_readers():
    """an upload that defers the planes, then readers that need counts (from the slots), nothing, planes, all planes"""
    return [("set_prep", "zero"), ("upload", 0, "low", 700, 3000, 71, False), ("expect", "planes_stored", 0, False),
            ("set_ids", 0, "d"), ("set_path", "consensus"), ("text_square", "tn93", 0, 6), ("run_square", "k80", 0, 64, False),
            ("expect", "planes_stored", 0, False), ("base_counts", 0), ("differences", 0), ("expect", "planes_stored", 0, True),
            ("set_path", "dense"), ("run_square", "tn93", 0, 64, False), ("run_square", "raw", 640, 700, True),
            ("set_path", "consensus"), ("run_square", "tn93", 0, 64, False), ("run_square", "jc69", 640, 700, False),
            ("expect", "last_path", "consensus")]


def features_between_runs():
    """bootstrap (its own set, ctx->boot), nearest, clusters, matrix text and NJ between two square and two rectangle runs:
    slots, ids and run records stay as they were"""
    ops = [("set_prep", "zero"), ("upload", 0, "clade_runs", 300, 4100, 81, False), ("upload", 1, "low", 100, 4100, 82, False),
           ("set_ids", 0, "a"), ("set_ids", 1, "b"), ("set_path", "consensus"), ("expect", "run_records", 0, True)]
    features = [("nj_bootstrap", "n_high", 3, 5), ("nearest", "tn93", 4, True, 0, 1), ("clusters", "k80", 0.01), ("nj", "n_high"),
                ("text_matrix", "tn93", True, 0, 1, 0, 30, "tsv")]
    for run in (("run_square", "k80", 0, 300, False), ("run_rect", "tn93", 0, 1, 0, 300, False)):
        for f in features:
            # the matrix text runs slot 0 against itself as a rectangle (the diagonal is part of it): like any run that is
            # no square it has the stripped lists of its column set rebuilt whole (run_sets), so the run records go and the
            # planes are written — the answers stay.  Found by this sequence; every other feature leaves the state alone.
            moved = f[0] == "text_matrix" and run[0] == "run_square"
            ops += [run, ("snapshot",), f, ("expect", "run_records", 0, False) if moved else ("expect", "unchanged"), run,
                    ("text_square", "raw", 0, 3)]
    return ops


def stream_between_squares():
    """a stream pipeline and a streamed batch between square runs on a stripped slot 0: the stream's column set is slot 0
    and its run is no square, so it drops the run records (run_sets: !square && cols.runs.active)"""
    sq = [("run_square", "k80", 0, 64, False), ("run_square", "tn93", 536, 600, True)]
    return ([("set_prep", "zero"), ("upload", 0, "runs", 600, 4100, 91, False), ("set_path", "consensus"),
             ("expect", "run_records", 0, True)] + sq +
            [("stream", "tn93", "low", 19, 8, 3, 92, False, False), ("expect", "run_records", 0, False)] + sq +
            [("set_path", "auto"), ("upload", 0, "runs", 600, 4100, 93, False), ("set_path", "consensus"), ("expect", "run_records", 0, True),
             ("stream", "k80", "low", 19, 4, 2, 94, True, True)] + sq +
            [("set_path", "auto"), ("upload", 0, "runs", 600, 4100, 95, False), ("set_path", "hybrid")] + sq +
            [("run_stream_batch", "raw", "low", 40, 96, False, True)] + sq)


def errors_in_the_middle():
    """after every error the next operation answers as if nothing had happened; a rejected upload leaves its slot not
    loaded (a clean DST_ERR_STATE on every use) and the other slot as it was"""
    sq = [("run_square", "k80", 0, 64, False)]
    return ([("set_prep", "zero"), ("upload", 0, "runs", 300, 4100, 101, False), ("upload", 1, "low", 65, 4100, 102, False),
             ("set_ids", 0, "e"), ("set_path", "consensus")] + sq +
            [("err_text_capacity", "tn93")] + sq + [("text_square", "tn93", 0, 3), ("err_width", 0), ("differences", 0),
             ("err_nj_nonfinite", "raw"), ("nj", "n_high"), ("clusters_tiny_slabs", "n_high", 3.0), ("clusters", "n_high", 3.0),
             ("bad_upload", 1, 65, 1000, 103), ("run_rect", "k80", 0, 1, 0, 300, False), ("base_counts", 1)] + sq +
            [("run_stream_batch", "k80", "low", 7, 104, False, False), ("run_rect", "k80", 0, 1, 0, 300, False),
             ("bad_upload", 0, 300, 1000, 105)] + sq + [("stream", "raw", "low", 5, 4, 2, 106, False, False), ("nearest", "raw", 1, True, 0, 1),
             ("text_square", "raw", 0, 2), ("upload", 0, "low", 300, 4100, 107, False)] + sq +
            [("run_rect", "tn93", 1, 0, 0, 7, False), ("text_square", "raw", 0, 2)])


def schedule_cache(path):
    """more row ranges than the context keeps tile schedules for (16), queued on one stream of the caller's, then the first
    range again (evicted and rebuilt in a recycled buffer)"""
    n = 1300
    b = [int(x) for x in np.linspace(0, n - 1, 20)]
    ranges = [("run_square_device", "raw", b[k], b[k + 1]) for k in range(19)]
    return ([("set_prep", "zero"), ("upload", 0, "clade", n, 2000, 111, False), ("set_path", path)] + ranges + [ranges[0], ranges[1]] +
            [("run_square", "k80", b[3], b[4], True), ("expect", "last_path", path)])


def stream_close_then_schedule_eviction(path):
    """The abort walk seed 53 found, as a fixed order.  A batch of a stream pipeline runs on the pipeline's own compute
    stream, so the tile schedule of its geometry (rectangle, rows [0, batch), slot 0's columns) is made with that stream as
    its user (prepare_schedule).  Closing the pipeline destroys the stream; the schedule stays.  It is the oldest of the
    context, so the 19 row ranges that follow — each a new geometry, 16 are kept — evict it, and the eviction waits for the
    schedule's users: on the destroyed handle the runtime ended the process.  The context now keeps a mark of the stream (an
    event of its own, dst_ctx::Mark) and no handle, and the eviction waits for that event; closing a pipeline tells the
    context nothing.  Then the first range again, and a second pipeline of the same geometry (its schedule rebuilt)."""
    n = 1300
    b = [int(x) for x in np.linspace(0, n - 1, 20)]
    ranges = [("run_square", "raw", b[k], b[k + 1], False) for k in range(19)]
    return ([("set_prep", "zero"), ("upload", 0, "clade", n, 2000, 121, False), ("set_path", path),
             ("stream", "k80", "low", 19, 8, 3, 122, False, False), ("run_stream_batch", "raw", "low", 40, 123, False, False)] +
            ranges + [ranges[0], ("stream", "k80", "low", 19, 8, 3, 124, True, True), ranges[1],
                      ("run_stream_batch", "tn93", "low", 7, 125, False, False), ("expect", "last_path", path)])


def page_locked_buffers_grow_and_are_reused():
    """The context's four page-locked buffers (links' chunk, pair sites' batch and window, the text's near ties) and the
    device buffers beside them through small, grow, small: 300 records, 1,300, 300 again, 2,000 sites each — the smallest
    order in which a grow that left a stale pointer or a stale capacity behind would show.  At each size the links within
    a threshold with values and tallies (tn93: the chunk is the slab's pair count, 44,850 then 844,350 entries), the
    difference sites of 64 pairs, and the tn93 text of 200 rows, whose near ties go through the fourth buffer; each
    answer is the pristine engine's."""
    ops = []
    for n, seed in ((300, 141), (1300, 142), (300, 143)):
        ops += [("upload", 0, "low", n, 2000, seed, False), ("set_ids", 0, "p%d_" % seed),
                ("links", "tn93", 0.004, True, 0, 1, True, True), ("pair_sites", "tn93", 64, True, 0, 1, seed),
                ("text_square", "tn93", 0, 200)]
    return ops


def more_streams_than_marks_used_to_hold():
    """Six streams of the caller's (torch's, from its pool, alive to the end: none is ever destroyed) on one context, which
    used to remember the runs of four: one row range per stream in turn on the consensus path, the measure changing on
    the way (every change of family rebuilds the per-record constants behind a wait for the other streams' marks), then
    other content into the same slot (the rebuild that must wait for all six) and the first range again.
    Every run is waited for before its answer is read, so no timing can make this fail reliably: what it holds is that
    the path with more than four streams runs at all, trims its marks, and stays correct."""
    n = 1300
    b = [int(x) for x in np.linspace(0, n - 1, 7)]
    ranges = [("run_square_device", WALK[k], b[k], b[k + 1], k) for k in range(6)]
    return ([("set_prep", "zero"), ("upload", 0, "clade", n, 2000, 131, False), ("set_path", "consensus")] + ranges +
            [("upload", 0, "clade", n, 2000, 132, False), ranges[0], ("expect", "last_path", "consensus")])


DIRECTED = {
    "advice_order_consensus": advice_order("consensus"),
    "advice_order_hybrid": advice_order("hybrid"),
    "path_walk_same_upload": path_walk(),
    "family_walk": family_walk(),
    "reference_ownership_consensus": reference_ownership("consensus"),
    "reference_ownership_hybrid": reference_ownership("hybrid"),
    "same_shape_new_content_then_smaller": same_shape_new_content(),
    "wide_narrow_wide": wide_narrow_wide(),
    "deferred_planes_alternating_readers": deferred_planes_readers(),
    "features_between_runs": features_between_runs(),
    "stream_between_squares": stream_between_squares(),
    "errors_in_the_middle": errors_in_the_middle(),
    "schedule_cache_dense": schedule_cache("dense"),
    "schedule_cache_consensus": schedule_cache("consensus"),
    "schedule_cache_hybrid": schedule_cache("hybrid"),
    "stream_close_then_schedule_eviction_dense": stream_close_then_schedule_eviction("dense"),
    "stream_close_then_schedule_eviction_consensus": stream_close_then_schedule_eviction("consensus"),
    "page_locked_buffers_grow_and_are_reused": page_locked_buffers_grow_and_are_reused(),
    "more_streams_than_marks_used_to_hold": more_streams_than_marks_used_to_hold(),
}
SEEDS = (53, 61, 92, 82, 1)       # chosen so that the coverage test below holds (a greedy search over seeds 1..199)
TOTALS = {"sequences": 0, "answers": 0, "state": 0, "values": 0}


def run_sequence(seq):
    answers, state, values = em.replay(seq)
    TOTALS["sequences"] += 1
    TOTALS["answers"] += answers
    TOTALS["state"] += state
    TOTALS["values"] += values
    # (a figure for the log, per sequence and running: shown with -s)
    print("\n%d operations answered as the oracle and a pristine engine do, %d uploads / knobs / ids followed by the model, "
          "%d values held to the oracle; so far %d sequences, %d + %d operations"
          % (answers, state, values, TOTALS["sequences"], TOTALS["answers"], TOTALS["state"]))


@gpu
@pytest.mark.parametrize("name", list(DIRECTED))
def test_directed_sequence(name):
    run_sequence(DIRECTED[name])


@gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_random_walk(seed):
    run_sequence(em.walk(seed))


def test_the_walks_are_deterministic_and_cover_the_vocabulary():
    walks = [em.walk(s) for s in SEEDS]
    assert walks == [em.walk(s) for s in SEEDS]
    assert all(25 <= len(w) <= 40 for w in walks), [len(w) for w in walks]
    for w in walks:
        for op in w:
            assert op[0] in em.OP_CLASS, op
            if op[0] in ("upload", "upload_device"):
                assert op[3] in em.WALK_N and op[4] in em.WALK_L and op[2] in em._kinds_for(op[3], op[4]), op
    names = {op[0] for w in walks for op in w}
    assert names == set(em.OP_CLASS), sorted(set(em.OP_CLASS) - names)
    pairs = set()
    for w in walks:
        classes = [em.op_class(op) for op in w]
        pairs |= set(zip(classes, classes[1:]))
    missing = sorted({(a, b) for a in em.CLASSES for b in em.CLASSES} - pairs)
    assert not missing, missing
    # the directed sequences use the same vocabulary (plus the operations only they name, and the introspection checks)
    assert not set(em.DIRECTED_OPS) & set(em.OP_CLASS) and set(em.DIRECTED_OPS.values()) <= set(em.CLASSES)
    for name, seq in DIRECTED.items():
        for op in seq:
            assert op[0] in em.OP_CLASS or op[0] in em.DIRECTED_OPS or op[0] in em.CHECKS, (name, op)
    assert set(em.DIRECTED_OPS) <= {op[0] for seq in DIRECTED.values() for op in seq}
    kinds = {op[2] for seq in list(DIRECTED.values()) + walks for op in seq if op[0] in ("upload", "upload_device")}
    assert kinds == set(em.KINDS), sorted(set(em.KINDS) - kinds)
    assert any(op[0] == "upload" and op[4] >= 65536 for seq in DIRECTED.values() for op in seq)
