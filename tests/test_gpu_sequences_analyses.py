"""The analyses and stream kinds added since test_gpu_sequences.py, held to call order on ONE engine.

The second vocabulary of tests/engine_model.py (ANALYSIS_OPS): mst, dendrogram, summary, group_summary, representatives,
links, run_pairs, pair_sites, run_windows, window_base_counts, nearest_windows, and dst_streams as handles that stay
open while the context does something else (plain, closest on either side, links, window-closest).  Every answer is
held, bit for bit, to a pristine engine on the dense path — a stream's to a pristine stream that was given slot 0 and the
same batches with nothing in between — and to the reference module of its analysis by the rule of that analysis's own
test module.  DIRECTED names the orders the shared buffers imply (dst_ctx::pair_slab, nn_lists, win_table / win_counts,
the page-locked staging buffers, deferred planes, run records); SEEDS are walks over the whole vocabulary
(engine_model.walk_analyses).  A failure prints the sequence up to the failing operation as a replay([...]) literal.

Without a GPU: the generator's conditions (test_the_analysis_walks_*).
"""
import pytest

import engine_model as em
from engine_model import replay   # noqa: F401  (what a failure's message names)

gpu = pytest.mark.gpu
INF = float("inf")


# ---------------------------------------------------------------------------------------------- one per shared buffer
def slab_users(big=0):
    """every user of dst_ctx::pair_slab, ordered so that the payload changes at every step: 8 bytes per pair, 16 bytes
    (tn93's four tally words), W words (k80: 3, raw: 2); a slab as large as the set allows, then max_pairs = 500 (dozens
    of slabs with a short last one), then large again"""
    return [("mst", "raw", big, False), ("nearest", "tn93", 3, True, 0, 1), ("summary", "k80", 0.004, True, 0, 1, 500, 16),
            ("mst", "tn93", 500, True), ("clusters", "n_high", 3.0), ("representatives", "k80", 0.004, big, True, True),
            ("dendrogram", "n", "average", 500), ("links", "tn93", 0.004, True, 0, 1, True, True, big),
            ("group_summary", "raw", 4, 7, 0.004, True, 0, 1, 500), ("run_pairs", "k80", 5000, True, 0, 1, 2, True, True, big, "sweep"),
            ("nj", "k80"), ("nearest_windows", "raw", "few", 2, True, 0, 1, True, 0), ("links", "n", 3.0, True, 0, 1, True, False, 500),
            ("run_pairs", "tn93", 64, True, 0, 1, 3, True, False, 500, "sweep")]


def slab_kinds_in_turn():
    """one upload, the list forwards and then backwards"""
    users = slab_users()
    return [("upload", 0, "low", 300, 1000, 201, False)] + users + users[::-1]


def slab_kinds_after_a_smaller_and_a_larger_set():
    """the same list after an upload of a smaller set (the slab keeps its size), then backwards after a larger one"""
    users = slab_users()
    return ([("upload", 0, "low", 300, 1000, 201, False), users[1], ("upload", 0, "low", 130, 1000, 202, False)] + users +
            [("upload", 0, "low", 420, 1000, 203, False)] + users[::-1])


def lists_two_layouts():
    """nn_lists serves dst_nearest, then holds another layout for dst_nearest_windows: K = 5, the windowed K = 2 with
    tallies, K = 1, the windowed rectangle — with a closest stream (lists of its own) open across the middle two"""
    return [("upload", 0, "low", 300, 1000, 211, False), ("upload", 1, "low", 65, 1000, 212, False),
            ("nearest", "tn93", 5, True, 0, 1),
            ("stream_open", "c", "closest_loaded", "tn93", 3, False, 40, 3), ("stream_push", "c", "low", 7, 213),
            ("nearest_windows", "tn93", "few", 2, True, 0, 1, True, 0), ("stream_push", "c", "diverse", 40, 214),
            ("nearest", "raw", 1, True, 0, 1), ("stream_pop", "c"), ("stream_pop", "c"), ("stream_result", "c", True),
            ("nearest_windows", "k80", "all", 2, False, 1, 0, False, 0), ("stream_push", "c", "low", 1, 215), ("stream_pop", "c"),
            ("stream_result", "c", True), ("stream_close", "c"), ("nearest", "tn93", 5, False, 0, 1),
            ("nearest_windows", "tn93", "other", 5, False, 0, 1, True, 200_000)]


def window_tables():
    """win_table and win_counts serve three calls (dst_window_base_counts reads win_counts as uint32): nine windows on
    tn93, three for the base counts, nine others, the first list again; a same-shape upload of new content and the first
    call again (stale per-window counts would show); then a rectangle whose column set is smaller than its row set"""
    first = ("run_windows", "tn93", "all", True, 0, 1, 0, 96, False)
    return [("upload", 0, "low", 300, 1000, 221, False), first, ("window_base_counts", 0, "few"),
            ("nearest_windows", "tn93", "other", 2, True, 0, 1, False, 0), first, ("run_windows", "tn93", "all", True, 0, 1, 204, 300, True),
            ("upload", 0, "low", 300, 1000, 222, False), first, ("nearest_windows", "tn93", "other", 2, True, 0, 1, True, 0),
            ("upload", 1, "low", 65, 1000, 223, False), ("run_windows", "tn93", "all", False, 0, 1, 0, 300, False),
            ("window_base_counts", 1, "all"), ("nearest_windows", "tn93", "other", 2, False, 0, 1, True, 0),
            ("run_windows", "tn93", "few", False, 1, 0, 0, 65, False), first]


def deferred_planes_new_readers(part):
    """An upload that defers the planes, then each new reader as the FIRST reader, one upload per reader, and what
    planes_stored says afterwards — read off the calls:
      run_windows (any measure: dst_run_windows calls ensure_derived for both sets)            -> stored
      window_base_counts (ensure_planes)                                                        -> stored
      run_pairs, three pairs (the direct kernel: prepare_direct -> ensure_planes / _derived)   -> stored
      run_pairs, 5,000 pairs without a diagonal one, swept (run_sets on the consensus path)    -> still deferred
      group_summary, representatives (walk_slabs -> run_sets, the square, the consensus path)  -> still deferred
      opening a window-closest stream (ensure_derived at open, as the header says)              -> stored
      opening a closest stream (nothing is read before the first submit)                        -> still deferred
    Then a square run on the consensus path, which must still be right."""
    readers = {
        "windows": [([("run_windows", "n", "all", True, 0, 1, 0, 64, True)], True),
                    ([("run_windows", "k80", "other", True, 0, 1, 636, 700, False)], True),
                    ([("window_base_counts", 0, "all")], True),
                    ([("nearest_windows", "raw", "few", 2, True, 0, 1, False, 0)], True)],
        "pairs": [([("run_pairs", "tn93", 3, True, 0, 1, 5, True, True, 0, "auto")], True),
                  ([("run_pairs", "tn93", 5000, True, 0, 1, 6, True, True, 0, "sweep")], False),
                  ([("group_summary", "tn93", 4, 9, 0.004, True, 0, 1, 0)], False),
                  ([("representatives", "k80", 0.004, 0, True, True)], False)],
        "streams": [([("stream_open", "w", "window_closest", "tn93", "all", 2, 0, False, 40, 3)], True),
                    ([("stream_open", "c", "closest_loaded", "tn93", 3, False, 40, 3)], False)],
    }[part]
    ops = [("set_prep", "zero")]
    for k, (reader, stored) in enumerate(readers):
        ops += [("set_path", "auto"), ("upload", 0, "low", 700, 3000, 231 + k, False), ("expect", "planes_stored", 0, False),
                ("set_path", "consensus")] + reader + [("expect", "planes_stored", 0, stored)]
        if reader[0][0] == "stream_open":
            tag = reader[0][1]
            ops += [("stream_push", tag, "low", 7, 241 + k), ("stream_pop", tag), ("stream_result", tag, True), ("stream_close", tag)]
        ops += [("run_square", "k80", 0, 64, False), ("run_square", "tn93", 636, 700, True), ("expect", "last_path", "consensus")]
    return ops


def run_records_and_the_new_calls(path, part):
    """like features_between_runs: a set with stripped run records, every new analysis between two square runs (part
    "square") and between two rectangle runs (part "rect")"""
    kind = "clade_runs"
    ops = [("set_prep", "zero"), ("upload", 0, kind, 300, 4100, 251, False), ("upload", 1, "low", 100, 4100, 252, False),
           ("set_path", path), ("expect", "run_records", 0, True)]
    still = [("mst", "tn93", 0, True), ("dendrogram", "n", "complete", 0), ("summary", "k80", 0.004, True, 0, 1, 0, 16),
             ("group_summary", "tn93", 4, 3, 0.004, True, 0, 1, 20_000), ("representatives", "raw", 0.004, 0, True, False),
             ("links", "k80", 0.004, True, 0, 1, True, True, 0), ("run_pairs", "tn93", 5000, True, 0, 1, 8, True, True, 0, "sweep")]
    # the window calls and the direct kernel of run_pairs read the planes: the first of them has the deferred planes
    # written (ensure_derived / ensure_planes), and that is all — the lists and the run records stay as they were
    movers = [("run_windows", "tn93", "all", True, 0, 1, 0, 64, False), ("window_base_counts", 0, "few"),
              ("nearest_windows", "k80", "other", 2, True, 0, 1, True, 0), ("run_pairs", "k80", 64, True, 0, 1, 9, True, True, 0, "direct"),
              ("pair_sites", "raw", 64, True, 0, 1, 10)]
    sq, rect = ("run_square", "k80", 0, 96, False), ("run_rect", "tn93", 0, 1, 204, 300, False)
    if part == "square":
        ops.append(sq)
        for f in still:
            ops += [("snapshot",), f, ("expect", "unchanged"), sq]
        for k, f in enumerate(movers):
            ops += [("snapshot",), f, ("expect", "planes_stored", 0, True) if k == 0 else ("expect", "unchanged"),
                    ("expect", "run_records", 0, True), sq]
        return ops + [("run_square", "tn93", 204, 300, True)]
    # the first rectangle run has slot 0's lists made against slot 1's reference, from the planes and therefore whole
    # (ensure_index: "lists from the planes keep every entry"): the run records go and the planes are written, once
    ops += [rect, ("expect", "run_records", 0, False), ("expect", "planes_stored", 0, True), sq, rect]
    for f in still + movers:       # every one of them: the planes are stored by now, so none moves anything
        ops += [("snapshot",), f, ("expect", "unchanged"), rect]
    # then slot 0 as the COLUMN set of a run that is no square, here the rectangle form of summary (with run records it
    # would have its stripped lists rebuilt whole: run_sets, !square && cols.runs.active), a new upload, and the same
    # call as the first that is no square after it: the run records go with it, whoever asks
    ops += [("summary", "k80", 0.004, False, 1, 0, 0, 16), ("expect", "run_records", 0, False), rect, sq,
            ("upload", 0, kind, 300, 4100, 253, False), ("expect", "run_records", 0, True), sq,
            ("summary", "k80", 0.004, False, 1, 0, 0, 16), ("expect", "run_records", 0, False), sq]
    return ops


def page_locked_small_grow_small():
    """page_locked_buffers_grow_and_are_reused for the buffers added since (rp_batch_host, group_host, links_host, the
    links stream's windows): 300 records, 1,300, 300 again, 2,000 sites each"""
    ops = []
    for n, seed in ((300, 261), (1300, 262), (300, 263)):
        ops += [("upload", 0, "low", n, 2000, seed, False), ("run_pairs", "tn93", 5000, True, 0, 1, seed, True, True, 0, "auto"),
                ("group_summary", "tn93", 4, seed, 0.004, True, 0, 1, 0), ("links", "tn93", 0.004, True, 0, 1, True, True, 0),
                # every pair of the batch links (7 x n): windows of 16, so all but the first are written after collect
                ("stream_open", "l", "links", "raw", INF, True, True, 16, False, 40, 2), ("stream_push", "l", "low", 7, seed + 10),
                ("stream_pop", "l"), ("stream_close", "l")]
    return ops


def between(tags, k, seed):
    """one batch into each open stream, then each collected"""
    return ([("stream_push", t, ("low", "diverse")[(k + i) % 2], (7, 1, 40)[(k + i) % 3], seed + 10 * k + i) for i, t in enumerate(tags)] +
            [("stream_pop", t) for t in tags])


def streams_open_across_everything():
    """a closest stream (loaded side) and a links stream stay open on a stripped slot 0 while the context uploads the
    other slot, changes path and preparation, runs squares, rectangles and analyses and formats text.  Their first batch
    is a run that is no square over slot 0 as the column set: the run records go (run_sets), as for any stream."""
    tags = ("c", "l")
    ops = [("set_prep", "zero"), ("upload", 0, "runs", 300, 4100, 271, False), ("set_path", "consensus"), ("expect", "run_records", 0, True),
           ("stream_open", "c", "closest_loaded", "tn93", 3, False, 40, 3),
           ("stream_open", "l", "links", "tn93", 0.004, True, True, 0, True, 40, 3)]
    ops += between(tags, 0, 272) + [("expect", "run_records", 0, False)]
    others = [("upload", 1, "low", 65, 4100, 273, False), ("set_path", "hybrid"), ("set_path", "dense"), ("set_path", "consensus"),
              ("set_prep", "default"), ("run_square", "raw", 0, 64, False), ("run_rect", "k80", 0, 1, 236, 300, False),
              ("nearest", "k80", 5, True, 0, 1), ("summary", "jc69", 0.004, True, 0, 1, 20_000, 16), ("set_ids", 0, "s"),
              ("text_square", "tn93", 0, 3)]
    for k, other in enumerate(others):
        ops += [other] + between(tags, k + 1, 272)
        if k == 5:
            ops += [("snapshot",), ("stream_result", "c", True), ("expect", "unchanged")]
    return ops + [("snapshot",), ("stream_result", "c", True), ("stream_result", "c", False), ("expect", "unchanged"),
                  ("stream_close", "c"), ("stream_close", "l"), ("run_square", "tn93", 0, 64, False)]


def window_closest_across_everything():
    """the same for two window-closest streams — tn93 (the loaded set's per-window counts are built once at open; every
    submit relies on ensure_derived being a no-op) and raw — with the context's own window calls on other lists between"""
    tags = ("w", "r")
    ops = [("set_prep", "zero"), ("upload", 0, "runs", 300, 4100, 281, False), ("set_path", "consensus"),
           ("stream_open", "w", "window_closest", "tn93", "all", 2, 0, False, 40, 3),
           ("stream_open", "r", "window_closest", "raw", "few", 3, 50_000, True, 40, 2)]
    ops += between(tags, 0, 282)
    others = [("upload", 1, "low", 65, 4100, 283, False), ("run_windows", "tn93", "other", True, 0, 1, 0, 64, False),
              ("set_path", "hybrid"), ("nearest_windows", "tn93", "few", 3, True, 0, 1, True, 0), ("window_base_counts", 0, "other"),
              ("set_path", "dense"), ("run_square", "k80", 0, 64, False), ("set_path", "consensus"),
              ("run_windows", "k80", "few", False, 1, 0, 0, 65, True), ("nearest_windows", "raw", "other", 2, False, 0, 1, False, 200_000),
              ("set_prep", "default"), ("run_rect", "tn93", 1, 0, 0, 65, False)]
    for k, other in enumerate(others):
        ops += [other] + between(tags, k + 1, 282)
        if k == 5:
            ops += [("snapshot",), ("stream_result", "w", True), ("stream_result", "r", True), ("expect", "unchanged")]
    return ops + [("snapshot",), ("stream_result", "w", True), ("stream_result", "w", False), ("stream_result", "r", True),
                  ("expect", "unchanged"), ("stream_close", "w"), ("stream_close", "r"), ("run_windows", "tn93", "all", True, 0, 1, 0, 64, False)]


def plain_and_window_closest_together():
    """the header forbids nothing about two dst_streams on one context: a plain stream (both outputs in turn) and a
    window-closest stream open together, their pushes interleaved, two batches of each in flight"""
    return [("upload", 0, "low", 300, 1000, 291, False),
            ("stream_open", "p", "plain", "tn93", False, True, 40, 3), ("stream_open", "w", "window_closest", "tn93", "all", 2, 0, False, 40, 3),
            ("stream_push", "p", "low", 7, 292), ("stream_push", "w", "diverse", 40, 293), ("stream_push", "w", "low", 1, 294),
            ("stream_push", "p", "diverse", 40, 295), ("stream_pop", "w"), ("stream_pop", "p"), ("stream_pop", "p"), ("stream_pop", "w"),
            ("stream_result", "w", True), ("stream_open", "q", "plain", "k80", True, False, 40, 2),
            ("stream_push", "q", "low", 7, 296), ("stream_push", "w", "low", 7, 297), ("stream_push", "p", "low", 1, 298),
            ("stream_pop", "p"), ("stream_pop", "w"), ("stream_pop", "q"), ("stream_close", "p"), ("stream_result", "w", True),
            ("stream_open", "s", "closest_streamed", "k80", 5, True, 40, 2), ("stream_push", "s", "diverse", 40, 299),
            ("stream_push", "w", "low", 1, 300), ("stream_pop", "s"), ("stream_pop", "w"), ("stream_push", "s", "low", 7, 289),
            ("stream_pop", "s"), ("stream_result", "w", False), ("stream_close", "s"),
            ("stream_close", "w"), ("stream_close", "q"), ("run_square", "tn93", 0, 64, False)]


def slot_0_changed_under_open_streams():
    """The one sequence that uploads to slot 0 under an open stream: the documented DST_ERR_STATE at the next submit when
    the record count changed (a links stream) and when the record count or the width changed (a window-closest stream);
    afterwards the context answers as ever.  (A re-upload of the same shape is outside the contract: the check sees the
    shape only.)"""
    return [("upload", 0, "low", 300, 1000, 301, False), ("stream_open", "l", "links", "tn93", 0.004, True, False, 0, False, 40, 3),
            ("stream_open", "w", "window_closest", "raw", "few", 2, 0, False, 40, 3)] + between(("l", "w"), 0, 302) + [
            ("upload", 0, "low", 130, 1000, 303, False), ("stream_push", "l", "low", 7, 304), ("stream_push", "w", "low", 7, 305),
            ("stream_close", "l"), ("stream_close", "w"), ("run_square", "tn93", 0, 130, False),
            ("links", "tn93", 0.004, True, 0, 1, True, False, 0),
            ("stream_open", "v", "window_closest", "tn93", "few", 2, 0, False, 40, 3)] + between(("v",), 1, 302) + [
            ("upload", 0, "low", 130, 129, 306, False), ("stream_push", "v", "low", 7, 307), ("stream_close", "v"),
            ("run_square", "tn93", 0, 130, False), ("nearest_windows", "tn93", "few", 2, True, 0, 1, True, 0),
            ("stream_open", "u", "window_closest", "tn93", "few", 2, 0, False, 40, 3)] + between(("u",), 2, 302) + [
            ("stream_result", "u", True), ("stream_close", "u")]


def errors_in_the_middle_new_calls():
    """one clean refusal per new call, each followed by a correct answer of the same call and of a square run.  (dst_links
    delivers through its sink and takes no capacity: there is no such refusal to ask for.)  A batch with an invalid code
    spoils that batch only on a links and on a plain stream and poisons the lists of a closest stream; neither disturbs
    another open stream or the context."""
    sq = [("run_square", "k80", 0, 64, False)]
    return ([("set_prep", "zero"), ("upload", 0, "runs", 300, 4100, 311, False), ("upload", 1, "low", 65, 4100, 312, False),
             ("set_path", "consensus")] + sq +
            [("err_pairs_index", "tn93"), ("run_pairs", "tn93", 64, True, 0, 1, 7, True, True, 0, "auto")] + sq +
            [("err_window", "reversed"), ("err_window", "past"), ("run_windows", "n", "all", True, 0, 1, 0, 64, True)] + sq +
            [("err_label", "k80"), ("group_summary", "k80", 4, 5, 0.004, True, 0, 1, 0)] + sq +
            [("err_capacity", "raw"), ("err_k", "raw", 0), ("err_k", "raw", 257), ("nearest_windows", "raw", "few", 2, True, 0, 1, False, 0)] + sq +
            [("err_dendrogram_nonfinite", "raw"), ("dendrogram", "n", "weighted", 0)] + sq +
            [("stream_open", "c", "closest_loaded", "k80", 3, False, 40, 3), ("stream_open", "l", "links", "k80", 0.004, True, True, 0, False, 40, 3),
             ("stream_open", "p", "plain", "k80", False, False, 40, 3)] + between(("c", "l", "p"), 0, 313) +
            [("stream_result", "c", True, 1), ("stream_result", "c", True),
             ("stream_push_bad", "l", "low", 7, 314), ("stream_pop", "l")] + between(("l", "p"), 1, 313) +
            [("stream_push_bad", "p", "low", 7, 315), ("stream_pop", "p"), ("stream_push", "c", "low", 7, 316),
             ("stream_result", "c", True), ("stream_pop", "c"), ("stream_push_bad", "c", "low", 7, 317), ("stream_pop", "c"),
             ("stream_push", "c", "low", 7, 318), ("stream_result", "c", True)] + between(("p", "l"), 2, 313) + sq +
            [("stream_close", "c"), ("stream_close", "l"), ("stream_close", "p")] + sq)


def wide_form():
    """one upload of 66,560 sites (the 32-bit tally form): windows across site 65,535 / 65,536 in run_windows and
    nearest_windows, run_pairs, and a window-closest stream of two batches.  The only sequence at that width."""
    return [("upload", 0, "wide", 96, 66_560, 321, False), ("run_windows", "tn93", "wide", True, 0, 1, 0, 96, True),
            ("run_windows", "k80", "wide", True, 0, 1, 32, 96, False), ("nearest_windows", "raw", "wide", 2, True, 0, 1, True, 0),
            ("run_pairs", "tn93", 64, True, 0, 1, 5, True, True, 0, "auto"), ("run_pairs", "k80", 64, True, 0, 1, 6, True, True, 500, "sweep"),
            ("stream_open", "w", "window_closest", "tn93", "wide", 2, 0, False, 8, 3), ("stream_push", "w", "low", 7, 322),
            ("window_base_counts", 0, "wide"), ("stream_push", "w", "low", 1, 323), ("stream_pop", "w"), ("stream_pop", "w"),
            ("stream_result", "w", True), ("stream_close", "w"), ("run_square", "tn93", 0, 96, True)]


DIRECTED = {
    "slab_kinds_in_turn": slab_kinds_in_turn(),
    "slab_kinds_after_a_smaller_and_a_larger_set": slab_kinds_after_a_smaller_and_a_larger_set(),
    "lists_two_layouts": lists_two_layouts(),
    "window_tables": window_tables(),
    "deferred_planes_new_readers_windows": deferred_planes_new_readers("windows"),
    "deferred_planes_new_readers_pairs": deferred_planes_new_readers("pairs"),
    "deferred_planes_new_readers_streams": deferred_planes_new_readers("streams"),
    "run_records_and_the_new_calls_consensus_square": run_records_and_the_new_calls("consensus", "square"),
    "run_records_and_the_new_calls_consensus_rect": run_records_and_the_new_calls("consensus", "rect"),
    "run_records_and_the_new_calls_hybrid_square": run_records_and_the_new_calls("hybrid", "square"),
    "run_records_and_the_new_calls_hybrid_rect": run_records_and_the_new_calls("hybrid", "rect"),
    "page_locked_small_grow_small": page_locked_small_grow_small(),
    "streams_open_across_everything": streams_open_across_everything(),
    "window_closest_across_everything": window_closest_across_everything(),
    "plain_and_window_closest_together": plain_and_window_closest_together(),
    "slot_0_changed_under_open_streams": slot_0_changed_under_open_streams(),
    "errors_in_the_middle_new_calls": errors_in_the_middle_new_calls(),
    "wide_form": wide_form(),
}
SEEDS = (174, 249, 51, 1, 3, 137)     # a greedy search over seeds 1..299 for the coverage test below, as for the first walks
TOTALS = {"sequences": 0, "answers": 0, "state": 0, "values": 0}
# operation name ("name kind" for a stream operation) -> held to [the pristine engine, the CPU oracle on the bytes, a
# reference module over the pristine engine's whole results]
COUNTS = {}


def run_sequence(seq):
    answers, state, values = em.replay(seq, analyses=True, counts=COUNTS)
    TOTALS["sequences"] += 1
    TOTALS["answers"] += answers
    TOTALS["state"] += state
    TOTALS["values"] += values
    # (figures for the log, per sequence and running: shown with -s)
    print("\n%d operations answered as the oracle and a pristine engine do, %d uploads / knobs / opens followed by the model, "
          "%d values held to the oracle; so far %d sequences, %d + %d operations"
          % (answers, state, values, TOTALS["sequences"], TOTALS["answers"], TOTALS["state"]))
    print("checked so far (pristine / oracle on the bytes / reference over pristine results): "
          + ", ".join("%s %d/%d/%d" % ((k,) + tuple(c)) for k, c in sorted(COUNTS.items())))


@gpu
@pytest.mark.parametrize("name", list(DIRECTED))
def test_directed_sequence(name):
    run_sequence(DIRECTED[name])


@gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_random_walk(seed):
    run_sequence(em.walk_analyses(seed))


# ---------------------------------------------------------------------------------------------- without a GPU
def stream_bookkeeping(seq, directed=False):
    """Follows the handles of a sequence: every stream operation names an open stream, no tag is opened twice at once, at
    most depth - 1 batches are in flight (depth when the sequence is a directed one), a collect has a batch to collect, and
    (a walk) slot 0 is not uploaded to while a stream is open.  Returns (kinds opened, tags open at the end, whether two
    pushes of one stream had an operation that is no stream operation between them)."""
    open_, kinds, apart, last_push, k = {}, set(), False, {}, 0
    for k, op in enumerate(seq):
        name = op[0]
        if name in ("upload", "upload_device") and op[1] == 0 and not directed:
            assert not open_, ("an upload to slot 0 under an open stream", k, op)
        if name not in em.STREAM_OPS:
            continue
        tag = op[1]
        if name == "stream_open":
            assert tag not in open_ and op[2] in em.STREAM_KINDS, (k, op)
            open_[tag] = [op[-1], 0]
            kinds.add(op[2])
            last_push.pop(tag, None)
            continue
        assert tag in open_, ("a stream operation on a closed stream", k, op)
        depth, flying = open_[tag]
        if name in ("stream_push", "stream_push_bad"):
            assert op[2] in ("low", "diverse") and op[3] in em.AWALK_BATCH, op
            if not directed:
                assert flying < depth - 1, ("a full ring", k, op)
            open_[tag][1] += 1
            if tag in last_push and any(o[0] not in em.STREAM_OPS and o[0] not in em.CHECKS for o in seq[last_push[tag] + 1:k]):
                apart = True
            last_push[tag] = k
        elif name == "stream_pop":
            assert flying > 0 or directed, ("nothing to collect", k, op)
            open_[tag][1] = max(flying - 1, 0)
        elif name == "stream_close":
            del open_[tag]
    return kinds, set(open_), apart


def test_the_analysis_walks_are_deterministic_and_cover_the_new_vocabulary():
    walks = [em.walk_analyses(s) for s in SEEDS]
    assert walks == [em.walk_analyses(s) for s in SEEDS]
    assert all(25 <= len(w) <= 40 for w in walks), [len(w) for w in walks]
    for w in walks:
        for op in w:
            assert op[0] in em.ANALYSIS_OPS, op
            if op[0] in ("upload", "upload_device"):
                assert op[3] in em.AWALK_N and op[4] in em.AWALK_L and op[2] in em._kinds_for(op[3], op[4]), op
    names = {op[0] for w in walks for op in w}
    assert names == set(em.ANALYSIS_OPS), sorted(set(em.ANALYSIS_OPS) - names)
    assert set(em.NEW_OPS) <= names
    pairs = set()
    for w in walks:
        classes = [em.analysis_class(op) for op in w]
        pairs |= set(zip(classes, classes[1:]))
    missing = sorted({(a, b) for a in em.ANALYSIS_CLASSES for b in em.ANALYSIS_CLASSES} - pairs)
    assert not missing, missing
    # the streams: every kind opened, a stream open across other operations, none used after its close, slot 0 left alone
    books = [stream_bookkeeping(w) for w in walks]
    assert set().union(*(b[0] for b in books)) == set(em.STREAM_KINDS)
    assert any(b[2] for b in books), "no walk has two pushes of one stream with another operation between them"
    # (a stream is closed by its walk or still open at the end, where the runner closes it: both happen)
    assert any(b[1] for b in books) and any(op[0] == "stream_close" for w in walks for op in w)
    # every call that takes max_pairs is given 0, 500 and something larger; every window menu and linkage is drawn
    at = {"mst": 2, "dendrogram": 3, "summary": 6, "group_summary": 8, "representatives": 3, "links": 8, "run_pairs": 9}
    drawn = {name: {op[k] for w in walks for op in w if op[0] == name} for name, k in at.items()}
    assert all(v and v <= {0, 500, 20_000} for v in drawn.values()), drawn
    assert set().union(*drawn.values()) == {0, 500, 20_000}, drawn
    assert {op[2] for w in walks for op in w if op[0] in ("run_windows", "nearest_windows")} == {"all", "other", "few"}
    assert {op[2] for w in walks for op in w if op[0] == "dendrogram"} <= set(em.LINKAGES)
    assert {op[3] for w in walks for op in w if op[0] in ("stream_push", "stream_push_bad")} == set(em.AWALK_BATCH)


def test_the_directed_sequences_use_the_second_vocabulary():
    names = set()
    for name, seq in DIRECTED.items():
        for op in seq:
            assert op[0] in em.ANALYSIS_OPS or op[0] in em.OP_CLASS or op[0] in em.CHECKS, (name, op)
            if op[0] in ("upload", "upload_device"):
                n, L = op[3], op[4]
                assert n * L <= 1300 * 2000 or (L >= 65536 and n <= 160) or (n <= 900 and L <= 4100), (name, op)
        kinds, left, _ = stream_bookkeeping(seq, directed=True)
        assert not left, (name, left)
        names |= {op[0] for op in seq}
    assert set(em.NEW_OPS) <= names, sorted(set(em.NEW_OPS) - names)
    kinds = set().union(*(stream_bookkeeping(seq, directed=True)[0] for seq in DIRECTED.values()))
    assert kinds == set(em.STREAM_KINDS), kinds
    assert {op[2] for seq in DIRECTED.values() for op in seq if op[0] == "dendrogram"} == set(em.LINKAGES)
    # only one sequence uploads to slot 0 while a stream is open
    for name, seq in DIRECTED.items():
        open_ = set()
        for op in seq:
            if op[0] == "stream_open":
                open_.add(op[1])
            elif op[0] == "stream_close":
                open_.discard(op[1])
            elif op[0] in ("upload", "upload_device") and op[1] == 0 and open_:
                assert name == "slot_0_changed_under_open_streams", (name, op)


def test_the_window_menus_hold_what_they_promise():
    import numpy as np
    for L in em.AWALK_L + (66_560,):
        for which in ("all", "other", "few") + (("wide",) if L > 65_536 else ()):
            w = em.window_list(L, which)
            assert w.dtype == np.uint64 and (w[:, 0] <= w[:, 1]).all() and (w[:, 1] <= L).all(), (L, which)
        for which in ("all", "other"):
            w = em.window_list(L, which).astype(np.int64).tolist()
            assert len(w) == 9, (L, which)
            assert any(b == e for b, e in w), "an empty window"
            assert any(e - b == 1 for b, e in w), "one site"
            assert any(e == L and b > 0 for b, e in w), "one that ends at L"
            assert len({tuple(x) for x in w}) < len(w), "a repeat"
            assert any(a[0] < b[0] < a[1] and b[1] > b[0] for a in w for b in w), "two that overlap"
            if L > 129:
                assert any(b in (127, 128, 129) or e in (127, 128, 129) for b, e in w), "a cut at 127-129"
                assert any(b // 128 == (e - 1) // 128 and e - b > 1 for b, e in w), "one inside a chunk"
        assert em.window_list(L, "all")[0].tolist() == [0, L]
    w = em.window_list(66_560, "wide").tolist()
    assert any(b < 65_536 < e for b, e in w) and [65_535, 65_536] in w


def test_the_drawn_pair_lists_hold_a_repeat_both_orders_and_the_diagonal():
    row, col = em.pair_list(300, 300, 64, 7, True)
    assert (row[1], col[1]) == (row[0], col[0]) and row[3] > col[3] and row[2] == col[2] and (row < col).any()
    row, col = em.pair_list(300, 300, 5000, 6, True)      # an even seed: no diagonal pair, the sweep alone serves the list
    assert (row != col).all() and (row > col).any() and (row[1], col[1]) == (row[0], col[0])
    row, col = em.pair_list(65, 300, 64, 7, False)
    assert row.max() < 65 and col.max() < 300 and col.max() >= 65
