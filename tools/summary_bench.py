"""dst_summary timing: one JSON line per shape and setting on GPU 0, with dst_clusters at the same threshold
in the same session beside it as the yardstick (it walks the same slabs and reads them once).

    python tools/summary_bench.py [--steps 3] [--only NAME ...] [--out profiles/summary/summary_bench.jsonl]

Shapes: the tools/synth alignment at 10,000 x 30,000 and 50,000 x 30,000 (-m n at T = 5 with 256 bins of width 1, the
concentrated histogram; -m raw with 4,096 bins spread over the value range of a sample of rows) and a uniform set of
10,000 x 256 (-m n, width 1: the spread case).  Per line: ms per call (median of --steps calls after one warm-up) of a
per-record-only call, a histogram-only call, a call with both, and of dst_clusters.  The histogram kernel with and without
the wave aggregation: run the script twice, the second time with DST_SUMMARY_NO_AGGREGATION=1 in the environment (the
line's "aggregation" says which).  The kernels' own times come from a separate `rocprofv3 --kernel-trace --stats` run of
this script.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import distance_amd as da  # noqa: E402
from tools import synth  # noqa: E402

SHAPES = [("c2", "synth", 10_000, 30_000), ("c3", "synth", 50_000, 30_000), ("u2", "uniform", 10_000, 256)]   # name, kind, records, sites


def value_range(eng, codes, measure):
    """the largest finite value of every 97th record against the set"""
    rows = np.arange(0, len(codes), 97)
    eng.upload(1, np.ascontiguousarray(codes[rows]))
    sample = eng.run_rect(measure, 1, 0)
    return float(sample[np.isfinite(sample)].max())


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
        for name, kind, n, L in SHAPES:
            if args.only and name not in args.only:
                continue
            if kind == "synth":
                codes = synth.alignment(synth.SEED, n, L)
                settings = [("n", 5.0, 256, 1.0), ("raw", None, 4096, None)]
            else:
                from helpers import uniform_codes
                codes = uniform_codes(n, L, seed=5)
                settings = [("n", 5.0, 256, 1.0)]
            eng.upload(0, codes)
            for measure, t, bins, width in settings:
                if width is None:
                    top = value_range(eng, codes, measure)
                    width, t = top / (bins - 96), top / 100   # (the sample's range and a little more; about the closest 1 %)
                rec_ms, rec_min, rec = timed(lambda: eng.summary(measure, t), args.steps)
                hist_ms, hist_min, hist = timed(lambda: eng.summary(measure, t, bins=bins, width=width, per_record=False), args.steps)
                both_ms, both_min, both = timed(lambda: eng.summary(measure, t, bins=bins, width=width), args.steps)
                cl_ms, cl_min, (_, cl_links) = timed(lambda: eng.clusters(measure, t), args.steps)
                assert rec["links"] == hist["links"] == both["links"] == cl_links
                assert np.array_equal(hist["hist"], both["hist"]) and np.array_equal(rec["sum"].view(np.uint64), both["sum"].view(np.uint64))
                occupied = int((both["hist"] > 0).sum())
                line = json.dumps({
                    "shape": name, "kind": kind, "records": n, "sites": L, "measure": measure, "threshold": t, "bins": bins,
                    "width": width, "steps": args.steps, "pairs": both["pairs"], "links": both["links"],
                    "occupied_bins": occupied, "top_bin_share": round(float(both["hist"].max()) / max(both["pairs"], 1), 4),
                    "aggregation": "DST_SUMMARY_NO_AGGREGATION" not in os.environ,
                    "per_record_ms": round(rec_ms, 3), "per_record_ms_min": round(rec_min, 3),
                    "histogram_ms": round(hist_ms, 3), "histogram_ms_min": round(hist_min, 3),
                    "both_ms": round(both_ms, 3), "both_ms_min": round(both_min, 3),
                    "clusters_ms": round(cl_ms, 3), "clusters_ms_min": round(cl_min, 3), "path": eng.last_path(),
                })
                print(line, flush=True)
                if args.out:
                    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                    with open(args.out, "a") as fh:
                        fh.write(line + "\n")


if __name__ == "__main__":
    main()
