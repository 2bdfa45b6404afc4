"""dst_clusters timing: one JSON line per shape and threshold on GPU 0.

    python tools/clusters_bench.py [--steps 3] [--only NAME ...] [--max-pairs P]

Shapes: 50,000 x 30,000 raw and tn93, and 10,000 x 30,000 raw, on the tools/synth alignment.  Per shape three thresholds:
"none" (T = -1: no pair links, the link kernel only streams the payloads), "sparse" (the 1 % quantile of a sample of
rows: about 1 % of the pairs linked) and "dense" (the 99 % quantile: nearly every pair).  Per line: ms per
dst_clusters call (median of --steps calls after one warm-up), the pair kernels' share from dst_kernel_ms_mean (mean per
launch x slabs per call), and the rest of the call (init / link / final kernels, the label copy, host work) as the
difference.  The link kernel's own time comes from a separate `rocprofv3 --kernel-trace --stats` run of this script.
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

SHAPES = [   # name, records, sites, measure
    ("c3_raw", 50_000, 30_000, "raw"),
    ("c3_tn93", 50_000, 30_000, "tn93"),
    ("c2_raw", 10_000, 30_000, "raw"),
]


def thresholds(eng, codes, measure):
    """none / sparse / dense from the values of every 97th record against the set, its own pair left out."""
    rows = np.arange(0, len(codes), 97)
    eng.upload(1, np.ascontiguousarray(codes[rows]))
    sample = eng.run_rect(measure, 1, 0)
    sample[np.arange(len(rows)), rows] = np.nan
    v = sample[np.isfinite(sample)]
    return [("none", -1.0), ("sparse", float(np.quantile(v, 0.01))), ("dense", float(np.quantile(v, 0.99)))]


def slab_count(n, max_pairs):
    """Row slabs of one call: dst_clusters' cut (cut_row_slabs) of the triangle at max_pairs (0: 2^25) pairs."""
    bound, slabs, rb = max_pairs or 1 << 25, 0, 0
    while rb < n - 1:
        pairs, re = 0, rb
        while re < n and (re == rb or pairs + (n - re - 1) <= bound):
            pairs += n - re - 1
            re += 1
        slabs += pairs > 0
        rb = re
    return slabs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--max-pairs", type=int, default=0, help="slab bound (0: the library's default)")
    args = ap.parse_args()
    with da.Engine(0) as eng:
        for name, n, L, measure in SHAPES:
            if args.only and name not in args.only:
                continue
            codes = synth.alignment(synth.SEED, n, L)
            eng.upload(0, codes)
            for tname, t in thresholds(eng, codes, measure):
                eng.clusters(measure, t, args.max_pairs)   # warm-up: buffers, lists, schedules
                times, pair_totals, launches = [], [], 0
                for _ in range(args.steps):
                    eng.kernel_ms_mean(reset=True)
                    t0 = time.perf_counter()
                    labels, links = eng.clusters(measure, t, args.max_pairs)
                    times.append((time.perf_counter() - t0) * 1e3)
                    km = eng.kernel_ms_mean(reset=True)   # mean over this call's last (up to 64) pair launches
                    launches = slab_count(n, args.max_pairs)
                    pair_totals.append(km["pair_ms"] * launches)
                ms = float(np.median(times))
                pair_ms = float(np.median(pair_totals))
                print(json.dumps({
                    "shape": name, "records": n, "sites": L, "measure": measure, "threshold_kind": tname,
                    "threshold": t, "max_pairs": args.max_pairs, "steps": args.steps, "ms_per_call": round(ms, 3),
                    "ms_min": round(min(times), 3), "pair_launches_per_call": launches,
                    "pair_kernels_ms_per_call": round(pair_ms, 3), "rest_ms_per_call": round(ms - pair_ms, 3),
                    "links": links, "link_share": round(links / (n * (n - 1) / 2), 6),
                    "clusters": int(np.count_nonzero(labels == np.arange(n))), "path": eng.last_path(),
                }), flush=True)


if __name__ == "__main__":
    main()
