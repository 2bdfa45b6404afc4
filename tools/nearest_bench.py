"""dst_nearest timing: one JSON line per shape on GPU 0.

    python tools/nearest_bench.py [--steps 3] [--only NAME ...]

Shapes: 50,000 x 30,000 raw and tn93 with k = 10 on the tools/synth alignment, the same raw on its clade-structured and
N-run variants, and 10,000 x 30,000 raw.  Per shape: ms per dst_nearest call (median of --steps calls after one warm-up),
the pair kernels' share from dst_kernel_ms_mean (mean per launch x launches per call), and the rest of the call
(selection kernels, list copies, host work) as the difference.  The selection kernels' own times come from a separate
`rocprofv3 --kernel-trace --stats` run of this script (nearest_rows_kernel / nearest_cols_kernel / nearest_init_kernel).
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

SHAPES = [   # name, records, sites, measure, data kind
    ("c3_raw", 50_000, 30_000, "raw", "plain"),
    ("c3_tn93", 50_000, 30_000, "tn93", "plain"),
    ("c3_raw_clade", 50_000, 30_000, "raw", "clade"),
    ("c3_raw_nrun", 50_000, 30_000, "raw", "nrun"),
    ("c2_raw", 10_000, 30_000, "raw", "plain"),
]


def codes_of(n, L, kind):
    root = synth.root(synth.SEED, L)
    codes = synth.records(synth.SEED, root, 0, n)
    if kind == "clade":
        synth.apply_clades(codes, root, *synth.clade_plan(synth.SEED, n, L))
    elif kind == "nrun":
        synth.apply_nruns(codes, synth.nrun_plan(synth.SEED, n, L))
    return codes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--only", nargs="*", default=None)
    args = ap.parse_args()
    cache = {}
    with da.Engine(0) as eng:
        for name, n, L, measure, kind in SHAPES:
            if args.only and name not in args.only:
                continue
            if (n, L, kind) not in cache:
                cache.clear()
                cache[(n, L, kind)] = codes_of(n, L, kind)
                eng.upload(0, cache[(n, L, kind)])
            eng.nearest(measure, args.k)   # warm-up: buffers, lists, schedules
            times, pair_totals, launches = [], [], 0
            for _ in range(args.steps):
                eng.kernel_ms_mean(reset=True)
                t0 = time.perf_counter()
                idx, _vals = eng.nearest(measure, args.k)
                times.append((time.perf_counter() - t0) * 1e3)
                km = eng.kernel_ms_mean(reset=True)   # this call's launches (fewer than the ring's 64)
                pair_totals.append(km["pair_ms"] * km["pair_launches"])
                launches = km["pair_launches"]
            ms = float(np.median(times))
            pair_ms = float(np.median(pair_totals))
            km = {"pair_ms": pair_ms / max(launches, 1)}
            launches_per_call = launches
            print(json.dumps({
                "shape": name, "records": n, "sites": L, "measure": measure, "data": kind, "k": args.k,
                "steps": args.steps, "ms_per_call": round(ms, 3), "ms_min": round(min(times), 3),
                "pair_kernel_ms_mean": round(km["pair_ms"], 4), "pair_launches_per_call": launches_per_call,
                "pair_kernels_ms_per_call": round(pair_ms, 3), "rest_ms_per_call": round(ms - pair_ms, 3),
                "path": eng.last_path(), "index_checksum": int(idx.astype(np.uint64).sum()),
            }), flush=True)


if __name__ == "__main__":
    main()
