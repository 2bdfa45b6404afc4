"""Window-closest stream throughput: one JSON line per measure on GPU 0, tools/synth alignments.

    python tools/window_closest_bench.py [--measures n,tn93] [--batches 32] [--rounds 5]
                                         [--out profiles/window_closest/window_closest_bench.jsonl]

Shape: 16 loaded queries x 30,000 sites, the 146 windows of `--windows 1000 --step 200`, --batches batches of 1,024 streamed
records, K = 10, the 4-bit wire format.  Per line, in ONE process and alternating between the variants in every round (one
warm-up round of each first), streamed records per second as the median, the smallest and the largest of --rounds:
  stream     the window-closest stream (dst_stream_open_window_closest): acquire, copy the batch's nibbles into the
             page-locked buffer, submit, collect with depth - 1 batches in flight, and one result call at the end;
  per_batch  (a) the only way there was before: upload(1, batch) + nearest_windows(square = 0) per batch and a numpy merge of the
             lists by (key, ordinal).  Its index and values are compared with the stream's bitwise in the same run (`same`);
  closest    (b) the plain closest stream (dst_stream_open_closest, for the loaded records) at the same K, for scale: the same
             ring and pack, one whole-width pair kernel and one selection per batch instead of 146 windows.  Its result is
             another quantity; it is compared with itself across the rounds.
Two more figures say what bounds the stream, each the median of --rounds after the alternating rounds:
  fill       the host's part alone: the copies of the batches' nibbles into a page-locked buffer, nothing submitted;
  no_fill    the stream without it: every batch submitted from the slots' buffers as an earlier pass left them (valid
             nibbles of other batches), so the host link, the pack, the sweep and the merge remain.
A stream is opened before the clock starts and closed after it stops: its page-locked buffers are allocated once per
stream, and a stream is as long as the database.  Neither (a) nor (b) runs the new code.  The nibbles of every batch are made before the clock starts (the host's encoder
writes them straight into the page-locked buffer); (a) uploads the code bytes, as dst_upload takes them."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import distance_amd as da  # noqa: E402
from tools import synth  # noqa: E402

TOP = np.uint64(0xFFFFFFFFFFFFFFFF)
DEPTH = 3


def stats(xs):
    return {"median": round(float(np.median(xs)), 1), "min": round(float(min(xs)), 1), "max": round(float(max(xs)), 1)}


def keys(vals):
    """dst_nearest's sort key of DST_OUT_DISTANCE payloads"""
    if vals.dtype == np.int64:
        return vals.view(np.uint64) ^ np.uint64(1 << 63)
    b = vals.view(np.uint64)
    k = np.where((b >> np.uint64(63)) == 1, ~b, b | np.uint64(1 << 63))
    k[vals == 0] = np.uint64(1 << 63)
    k[np.isnan(vals)] = TOP
    return k


def through(st, nibbles, batch, fill=True):
    """every batch through an open stream, DEPTH - 1 in flight; fill=False: the slots' buffers as they are"""
    for b in range(0, len(nibbles), batch):
        if st.in_flight() == DEPTH - 1:
            st.pop()
        buf, _ = st.buffer()
        n = min(batch, len(nibbles) - b)
        if fill:
            buf[:n] = nibbles[b:b + n]
        st.submit(n)
    while st.in_flight():
        st.pop()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measures", default="n,tn93")
    ap.add_argument("--batches", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    args = ap.parse_args()
    L, n_loaded, batch, K = 30_000, 16, 1024, 10
    windows = da.sliding_windows(L, 1000, 200)
    nw = len(windows)
    n_streamed = args.batches * batch
    loaded = synth.alignment(synth.SEED ^ 1, n_loaded, L)
    streamed = synth.alignment(synth.SEED, n_streamed, L)
    nibbles = da.engine.Stream.to_nibbles(streamed)
    with da.Engine(0) as eng:
        eng.upload(0, loaded)
        for measure in args.measures.split(","):
            dtype = np.int64 if measure in da.INT_MEASURES else np.float64

            def timed(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                return n_streamed / (time.perf_counter() - t0), out

            def stream_round():
                with eng.window_closest_stream(measure, windows, K, batch, depth=DEPTH, nibbles=True) as st:
                    return timed(lambda: (through(st, nibbles, batch), st.result())[1])

            def per_batch_round():
                idx = np.zeros((n_loaded, nw, 0), np.uint32)
                val = np.zeros((n_loaded, nw, 0), dtype)
                for b in range(0, n_streamed, batch):
                    eng.upload(1, streamed[b:b + batch])
                    i, v = eng.nearest_windows(measure, windows, K, square=False)
                    idx = np.concatenate([idx, i + np.uint32(b)], axis=2)
                    val = np.concatenate([val, v], axis=2)
                    order = np.lexsort((idx, keys(val)), axis=2)[:, :, :K]     # ascending (key, ordinal)
                    idx, val = np.take_along_axis(idx, order, axis=2), np.take_along_axis(val, order, axis=2)
                return idx, val

            def closest_round():
                with eng.closest_stream(measure, K, batch, side="loaded", depth=DEPTH, nibbles=True) as st:
                    return timed(lambda: (through(st, nibbles, batch), st.result())[1])

            variants = (("stream", stream_round), ("per_batch", lambda: timed(per_batch_round)), ("closest", closest_round))
            first = {name: fn()[1] for name, fn in variants}   # warm-up: planes, tables, code objects
            rate = {name: [] for name, _ in variants}
            same_rounds = True
            for _ in range(args.rounds):   # alternating
                for name, fn in variants:
                    r, out = fn()
                    rate[name].append(r)
                    same_rounds &= all(a.tobytes() == b.tobytes() for a, b in zip(out, first[name]))
            same = all(a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
                       for a, b in zip(first["stream"], first["per_batch"]))
            s = {name: stats(rate[name]) for name, _ in variants}
            # what bounds the stream: the host's copies alone, and the stream without them
            pinned = torch.empty((batch, nibbles.shape[1]), dtype=torch.uint8).pin_memory().numpy()
            fill, no_fill = [], []
            with eng.window_closest_stream(measure, windows, K, batch, depth=DEPTH, nibbles=True) as st:
                through(st, nibbles, batch)   # every slot's buffer holds a batch from here on
                for _ in range(args.rounds):
                    t0 = time.perf_counter()
                    for b in range(0, n_streamed, batch):
                        pinned[:] = nibbles[b:b + batch]
                    fill.append(n_streamed / (time.perf_counter() - t0))
                    no_fill.append(timed(lambda: (through(st, nibbles, batch, fill=False), st.result())[1])[0])
            line = json.dumps({
                "loaded": n_loaded, "sites": L, "windows": nw, "batch": batch, "batches": args.batches, "streamed": n_streamed, "k": K,
                "measure": measure, "wire": "nibbles", "depth": DEPTH, "rounds": args.rounds, "same": bool(same),
                "same_across_rounds": bool(same_rounds), "stream_records_per_s": s["stream"],
                "per_batch_records_per_s": s["per_batch"], "closest_records_per_s": s["closest"],
                "stream_over_per_batch": round(s["stream"]["median"] / s["per_batch"]["median"], 2),
                "stream_over_closest": round(s["stream"]["median"] / s["closest"]["median"], 2),
                "fill_records_per_s": stats(fill), "no_fill_records_per_s": stats(no_fill),
                "host_link_bytes_per_record": nibbles.shape[1],
            })
            print(line, flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as fh:
                    fh.write(line + "\n")


if __name__ == "__main__":
    main()
