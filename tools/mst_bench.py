"""dst_mst timing: one JSON line per shape on GPU 0.

    python tools/mst_bench.py [--steps 3] [--only NAME ...] [--max-pairs P]

Shapes: 10,000 x 30,000 and 50,000 x 30,000, raw and tn93, on the tools/synth alignment ("synth") and on its
clade-structured form ("clade": a third of the records share substitutions at 2 % of the sites).  Per line: ms per dst_mst
call with values and tallies (median of --steps calls after one warm-up), the Boruvka rounds, the pair kernels' share from
dst_kernel_ms_mean (mean per launch x launches per call: slabs x (rounds + the last empty sweep, if any, + the tally
sweep)), and beside them the model of DESIGN.md 3l:

    rounds x (one pair-kernel pass over the triangle + one read of its payloads) + one tally sweep

with the pair-kernel pass measured here, in the same session, as slabs x the mean DST_OUT_DISTANCE launch of a
dst_clusters call at a threshold that links nothing (the same slabs, no union work), and the payload reads at
--read-gbps (default 4000 GB/s).  The scan kernels' own time comes from a separate `rocprofv3 --kernel-trace --stats`
run of this script.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import distance_amd as da  # noqa: E402
from tools import synth  # noqa: E402
from tools.clusters_bench import slab_count  # noqa: E402

SHAPES = [   # name, records, sites
    ("c2", 10_000, 30_000),
    ("c3", 50_000, 30_000),
]
MEASURES = ("raw", "tn93")
DATA = ("synth", "clade")


def make(data: str, n: int, L: int) -> np.ndarray:
    r = synth.root(synth.SEED, L)
    codes = synth.records(synth.SEED, r, 0, n)
    if data == "clade":
        synth.apply_clades(codes, r, *synth.clade_plan(synth.SEED, n, L))
    return codes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--only", nargs="*", default=None, help="names like c2_raw_synth")
    ap.add_argument("--max-pairs", type=int, default=0, help="slab bound (0: the library's default)")
    ap.add_argument("--read-gbps", type=float, default=4000.0, help="the model's rate for reading the payloads")
    args = ap.parse_args()
    with da.Engine(0) as eng:
        for sname, n, L in SHAPES:
            for data in DATA:
                wanted = [m for m in MEASURES if not args.only or f"{sname}_{m}_{data}" in args.only]
                if not wanted:
                    continue
                eng.upload(0, make(data, n, L))
                slabs = slab_count(n, args.max_pairs)
                pairs = n * (n - 1) // 2
                for measure in wanted:
                    # the pair kernels' pass over the triangle in these slabs, on its own
                    eng.clusters(measure, -1.0, args.max_pairs)
                    eng.kernel_ms_mean(reset=True)
                    eng.clusters(measure, -1.0, args.max_pairs)
                    pass_ms = eng.kernel_ms_mean(reset=True)["pair_ms"] * slabs
                    eng.mst(measure, args.max_pairs, tallies=True)   # warm-up: buffers, lists, schedules
                    times, pair_totals = [], []
                    for _ in range(args.steps):
                        eng.kernel_ms_mean(reset=True)
                        t0 = time.perf_counter()
                        edges, values, rounds, tal = eng.mst(measure, args.max_pairs, tallies=True)
                        times.append((time.perf_counter() - t0) * 1e3)
                        km = eng.kernel_ms_mean(reset=True)   # mean over this call's last (up to 64) pair launches
                        sweeps = rounds + (0 if len(edges) == n - 1 else 1)
                        pair_totals.append(km["pair_ms"] * slabs * (sweeps + 1))
                    ms = float(np.median(times))
                    read_ms = pairs * 8 / (args.read_gbps * 1e9) * 1e3
                    model = rounds * (pass_ms + read_ms) + pass_ms
                    print(json.dumps({
                        "shape": f"{sname}_{measure}_{data}", "records": n, "sites": L, "measure": measure, "data": data,
                        "max_pairs": args.max_pairs, "steps": args.steps, "ms_per_call": round(ms, 3),
                        "ms_min": round(min(times), 3), "rounds": rounds, "sweeps": sweeps,
                        "log2_n_ceil": math.ceil(math.log2(n)), "edges": int(len(edges)), "slabs": slabs,
                        "pair_kernels_ms_per_call": round(float(np.median(pair_totals)), 3),
                        "rest_ms_per_call": round(ms - float(np.median(pair_totals)), 3),
                        "pair_pass_ms": round(pass_ms, 3), "payload_read_ms_per_round": round(read_ms, 3),
                        "model_ms": round(model, 3), "ratio_to_model": round(ms / model, 3), "path": eng.last_path(),
                    }), flush=True)


if __name__ == "__main__":
    main()
