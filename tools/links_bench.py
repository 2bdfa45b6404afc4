"""dst_links timing: one JSON line per shape and setting on GPU 0, with dst_clusters at the same threshold
in the same session beside it as the yardstick (it walks the same slabs and reads them once).

    python tools/links_bench.py [--steps 3] [--only NAME ...] [--out profiles/links/links_bench.jsonl]

Shapes: the tools/synth alignment at 10,000 x 30,000 and 50,000 x 30,000.  Settings: -m n at T = 5, -m raw at the
threshold that links about 1 % of the pairs (the 1 % quantile of a sample of rows), and at 10,000 records T = inf, where
every pair is a link.  Per line: ms per call (median of --steps calls after one warm-up) of a count-only dst_links call,
of a call that hands values + tallies to a sink that only counts, and of dst_clusters; the links, their share of the
pairs and the sink calls.  The kernels' own times come from a separate `rocprofv3 --kernel-trace --stats` run of this
script.
"""
from __future__ import annotations

import argparse
import ctypes as C
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


def one_percent(eng, codes):
    """the raw threshold that links about 1 % of the pairs: from every 97th record against the set, its own pair left out"""
    rows = np.arange(0, len(codes), 97)
    eng.upload(1, np.ascontiguousarray(codes[rows]))
    sample = eng.run_rect("raw", 1, 0)
    sample[np.arange(len(rows)), rows] = np.nan
    return float(np.quantile(sample[np.isfinite(sample)], 0.01))


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
    lib = da.load()
    calls = []
    sink = da.LINKS_SINK(lambda user, first, count, row, col, val, tal: calls.append(int(count)) or 0)
    with da.Engine(0) as eng:
        for name, n, L in SHAPES:
            if args.only and name not in args.only:
                continue
            codes = synth.alignment(synth.SEED, n, L)
            eng.upload(0, codes)
            settings = [("n", "T5", 5.0), ("raw", "1pct", one_percent(eng, codes))]
            if n <= 10_000:
                settings.append(("n", "inf", float("inf")))
            for measure, tname, t in settings:
                m = da.MEASURES[measure]
                total = C.c_uint64()

                def full():
                    calls.clear()
                    eng._check(lib.dst_links(eng._h, m, 1, 0, 1, t, 0, 3, sink, None, C.byref(total)))
                    return int(total.value)

                count_ms, count_min, links = timed(lambda: eng.links(measure, t, count_only=True), args.steps)
                full_ms, full_min, delivered = timed(full, args.steps)
                cl_ms, cl_min, (_, cl_links) = timed(lambda: eng.clusters(measure, t), args.steps)
                assert links == delivered == cl_links == sum(calls)
                line = json.dumps({
                    "shape": name, "records": n, "sites": L, "measure": measure, "threshold_kind": tname, "threshold": t,
                    "steps": args.steps, "links": links, "link_share": round(links / (n * (n - 1) / 2), 6),
                    "count_only_ms": round(count_ms, 3), "count_only_ms_min": round(count_min, 3),
                    "values_tallies_ms": round(full_ms, 3), "values_tallies_ms_min": round(full_min, 3),
                    "sink_calls": len(calls), "clusters_ms": round(cl_ms, 3), "clusters_ms_min": round(cl_min, 3),
                    "path": eng.last_path(),
                })
                print(line, flush=True)
                if args.out:
                    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                    with open(args.out, "a") as fh:
                        fh.write(line + "\n")


if __name__ == "__main__":
    main()
