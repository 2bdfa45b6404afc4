"""dst_dendrogram timing: one JSON line per (shape, data, measure, linkage) on GPU 0, with dst_nj on the
same set in the same process as the yardstick.

    python tools/dendrogram_bench.py [--steps 1] [--sizes 2000 10000 50000] [--data synth clade] [--measures raw tn93]
                                     [--linkages average weighted complete] [--no-nj]

Sets: the tools/synth alignment ("synth") and its clade-structured form ("clade": a third of the records share
substitutions at 2 % of the sites) at 2,000 / 10,000 / 50,000 x 30,000.  Per line: ms per dst_dendrogram call (median of
--steps calls after one warm-up call, which the 50,000 shapes skip), row_scans, the fill's pair kernels from
dst_kernel_ms_mean (mean per launch x the launches it counted: one per row slab, at most the 64 most recent), ms of
dst_nj on the same set, and the model of the rounds: per round one merge (three rows of 8 n bytes) and
row_scans / (n - 1) row reads of at most 8 n bytes, at 5 TB/s, plus three launches per round at 2.5 us.  Per-kernel times are not this tool's: run it under `rocprofv3 --kernel-trace --stats`
(the program after `--`, no counters) for those.
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

SITES = 30_000
LAUNCH_US = 2.5


def make(data: str, n: int, L: int) -> np.ndarray:
    r = synth.root(synth.SEED, L)
    codes = synth.records(synth.SEED, r, 0, n)
    if data == "clade":
        synth.apply_clades(codes, r, *synth.clade_plan(synth.SEED, n, L))
    return codes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--sizes", type=int, nargs="*", default=[2_000, 10_000, 50_000])
    ap.add_argument("--data", nargs="*", default=["synth", "clade"])
    ap.add_argument("--measures", nargs="*", default=["raw", "tn93"])
    ap.add_argument("--linkages", nargs="*", default=["average", "weighted", "complete"])
    ap.add_argument("--no-nj", action="store_true")
    args = ap.parse_args()
    with da.Engine(0) as eng:
        for n in args.sizes:
            for data in args.data:
                eng.upload(0, make(data, n, SITES))
                for measure in args.measures:
                    nj_ms = None
                    if not args.no_nj:
                        if n < 50_000:
                            eng.nj(measure)
                        t0 = time.perf_counter()
                        eng.nj(measure)
                        nj_ms = (time.perf_counter() - t0) * 1e3
                    for linkage in args.linkages:
                        if n < 50_000:
                            eng.dendrogram(measure, linkage)   # warm-up: code objects, slab scratch
                        times, pair_totals, first, scans = [], [], None, 0
                        for _ in range(args.steps):
                            eng.kernel_ms_mean(reset=True)
                            t0 = time.perf_counter()
                            parent, length, height, scans = eng.dendrogram(measure, linkage, stats=True)
                            times.append((time.perf_counter() - t0) * 1e3)
                            km = eng.kernel_ms_mean(reset=True)
                            pair_totals.append(km["pair_ms"] * km["pair_launches"])
                            if first is None:
                                first = (parent, length)
                            else:
                                assert np.array_equal(first[0], parent)
                                assert np.array_equal(first[1].view(np.uint64), length.view(np.uint64))
                        ms = float(np.median(times))
                        merge_bytes = (n - 2) * 3 * 8 * n
                        scan_bytes = scans * 8 * n
                        fill_bytes = 3 * 8 * n * n / 2   # every payload read once and written twice (pair kernels apart)
                        launches_ms = 3 * (n - 1) * LAUNCH_US * 1e-3
                        model_ms = (merge_bytes + scan_bytes + fill_bytes) / 5e12 * 1e3 + launches_ms
                        print(json.dumps({
                            "records": n, "sites": SITES, "data": data, "measure": measure, "linkage": linkage,
                            "steps": args.steps, "ms_per_call": round(ms, 1), "ms_min": round(min(times), 1),
                            "row_scans": scans, "row_scans_per_round": round(scans / (n - 1), 2),
                            "fill_pair_kernels_ms": round(float(np.median(pair_totals)), 1),
                            "model_traffic_ms_at_5TBps": round(model_ms - launches_ms, 1),
                            "model_launches_ms": round(launches_ms, 1), "model_ms": round(model_ms, 1),
                            "ratio_to_model": round(ms / model_ms, 2),
                            "nj_ms": None if nj_ms is None else round(nj_ms, 1),
                            "nj_over_dendrogram": None if nj_ms is None else round(nj_ms / ms, 2),
                            "negative_lengths": int((length < 0).sum()), "path": eng.last_path(),
                        }), flush=True)


if __name__ == "__main__":
    main()
