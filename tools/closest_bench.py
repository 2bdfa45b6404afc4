"""Closest streams against the plain stream: one JSON line per shape and stream kind on GPU 0.

    python tools/closest_bench.py [--steps 3] [--only c4 c3] [--out profiles/closest/closest_bench.jsonl]

Shapes, each with k = 10, in one session:
  c4   tools/bench_c4.py's shape: 1,000 loaded x 5,000,000 bp, streamed batches of 64 records, -m n_high
  c3   50,000 loaded x 30,000, streamed batches of 4,096 records of the tools/synth alignment, -m n_high
Per shape three streams over the same page-locked batches (depth 3, the 4-bit wire format, ring slots filled in place as
bench_c4's h2d_inclusive figures): the plain DST_OUT_TALLY stream, which copies every batch's result matrix back, and the
closest stream of each side, which keeps it on the device and adds the selection.  pairs/s = streamed x loaded records
per second of wall time, median of --steps steps after one warm-up step.  The selection kernels' own times come from a
separate `rocprofv3 --kernel-trace --stats -- python tools/closest_bench.py` run (nearest_stream_cols_kernel,
nearest_rows_kernel, nearest_init_kernel).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import distance_amd as da  # noqa: E402
from tools import synth  # noqa: E402

SHAPES = {   # name: loaded records, sites, records per batch, batches per step, measure
    "c4": (1_000, 5_000_000, 64, 4, "n_high"),
    "c3": (50_000, 30_000, 4_096, 4, "n_high"),
}
K, DEPTH = 10, 3


def step(st, batches, fill):
    """every batch once through the ring; fill: copy the batch into its slot (warm-up), else re-send what the slot holds"""
    for b in batches:
        if st.in_flight() == st.depth - 1:
            st.pop(copy=False)
        buf, _ = st.buffer()
        if fill:
            buf[:len(b)] = b
        st.submit(len(b))
    while st.in_flight():
        st.pop(copy=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "closest", "closest_bench.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    threads = min(len(os.sched_getaffinity(0)), 16)
    with da.Engine(0) as eng, open(args.out, "a") as out:
        for name, (n_loaded, L, B, nb, measure) in SHAPES.items():
            if args.only and name not in args.only:
                continue
            root = synth.root(synth.SEED, L)
            eng.upload(0, synth.records(synth.SEED, root, 0, n_loaded, threads=threads))
            batches = [da.engine.Stream.to_nibbles(synth.records(synth.SEED, root, n_loaded + g * B, B, threads=threads))
                       for g in range(nb)]
            pairs = nb * B * n_loaded
            kinds = [("plain_tally", lambda: eng.stream(measure, B, depth=DEPTH, tallies=True, nibbles=True)),
                     ("closest_loaded", lambda: eng.closest_stream(measure, K, B, side="loaded", depth=DEPTH, nibbles=True)),
                     ("closest_streamed", lambda: eng.closest_stream(measure, K, B, side="streamed", depth=DEPTH, nibbles=True))]
            for kind, make in kinds:
                with make() as st:
                    step(st, batches, True)
                    step(st, batches, True)     # every ring slot holds a real batch before timing starts
                    times = []
                    for _ in range(args.steps):
                        t0 = time.perf_counter()
                        step(st, batches, False)
                        times.append(time.perf_counter() - t0)
                    check = int(st.result()[0].astype(np.uint64).sum()) if kind == "closest_loaded" else None
                el = float(np.median(times))
                line = json.dumps({"shape": name, "stream": kind, "loaded": n_loaded, "sites": L, "batch_records": B,
                                   "batches_per_step": nb, "measure": measure, "k": K, "depth": DEPTH, "wire": "nibbles",
                                   "steps": args.steps, "ms_per_step": round(el * 1e3, 3), "ms_min": round(min(times) * 1e3, 3),
                                   "pairs_per_s": pairs / el, "path": eng.last_path(), "index_checksum": check})
                print(line, flush=True)
                out.write(line + "\n")
                out.flush()


if __name__ == "__main__":
    main()
