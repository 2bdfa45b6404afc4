"""dst_group_summary timing: one JSON line per shape, measure and labelling on GPU 0, with dst_summary's
per-record call (no histogram) on the same set in the same session beside it as the yardstick: existing code that makes
the same slab reads.  Every figure is also given as a ratio to it.

    python tools/group_summary_bench.py [--steps 3] [--only NAME ...] [--out profiles/groups/group_summary_bench.jsonl]

Shapes: the tools/synth alignment at 10,000 x 30,000 and 50,000 x 30,000, -m n (T = 5) and -m raw (T = inf).  Labellings:
3 large groups of contiguous records; the same 3 groups interleaved record by record; 1,000 groups of equal size,
interleaved.  Per line: ms per call (median of --steps calls after one warm-up) of a cells-only call and of a call with the
per-record tables.  The row kernel with and without its wave aggregation: run the script twice, the second time with
DST_GROUPS_NO_AGGREGATION=1 in the environment (the line's "aggregation" says which).  The kernels' own times come from a
separate `rocprofv3 --kernel-trace --stats` run of this script.
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

SHAPES = [("c2", 10_000, 30_000), ("c3", 50_000, 30_000)]   # name, records, sites
SETTINGS = [("n", 5.0), ("raw", float("inf"))]


def labellings(n):
    return [("3 contiguous", np.minimum(np.arange(n) // -(-n // 3), 2), 3), ("3 interleaved", np.arange(n) % 3, 3),
            ("1000 interleaved", np.arange(n) % 1000, 1000)]


def timed(fn, steps):
    fn()   # warm-up: buffers, lists, schedules
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        out = fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), float(min(times)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    args = ap.parse_args()
    with da.Engine(0) as eng:
        for name, n, L in SHAPES:
            if args.only and name not in args.only:
                continue
            eng.upload(0, synth.alignment(synth.SEED, n, L))
            for measure, t in SETTINGS:
                yard_ms, yard_min, yard = timed(lambda: eng.summary(measure, t), args.steps)
                for what, groups, G in labellings(n):
                    cells_ms, cells_min, cells = timed(lambda: eng.group_summary(measure, groups, G, t), args.steps)
                    rec_ms, rec_min, rec = timed(lambda: eng.group_summary(measure, groups, G, t, per_record=True), args.steps)
                    upper = np.triu(np.ones((G, G), bool))
                    assert int(cells["links"][upper].sum()) == int(rec["links"][upper].sum()) == yard["links"]
                    assert int(cells["summable_pairs"][upper].sum()) == yard["summable_pairs"]
                    assert np.array_equal(rec["rec_within"].sum(axis=1, dtype=np.uint32), yard["within"])
                    line = json.dumps({
                        "shape": name, "records": n, "sites": L, "measure": measure, "threshold": t, "labelling": what, "groups": G,
                        "steps": args.steps, "pairs": yard["pairs"], "aggregation": "DST_GROUPS_NO_AGGREGATION" not in os.environ,
                        "summary_per_record_ms": round(yard_ms, 3), "summary_per_record_ms_min": round(yard_min, 3),
                        "cells_ms": round(cells_ms, 3), "cells_ms_min": round(cells_min, 3),
                        "per_record_ms": round(rec_ms, 3), "per_record_ms_min": round(rec_min, 3),
                        "cells_ratio": round(cells_ms / yard_ms, 3), "per_record_ratio": round(rec_ms / yard_ms, 3),
                        "path": eng.last_path(),
                    })
                    print(line, flush=True)
                    if args.out:
                        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                        with open(args.out, "a") as fh:
                            fh.write(line + "\n")


if __name__ == "__main__":
    main()
