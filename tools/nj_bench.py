"""dst_nj timing: one JSON line per shape on GPU 0.

    python tools/nj_bench.py [--steps 1] [--only NAME ...]

Shapes: 2,000 / 10,000 / 50,000 x 30,000 raw and 50,000 x 30,000 tn93, on the tools/synth alignment.  Per line: ms per
dst_nj call (median of --steps calls after one warm-up call, which the 50,000 shapes skip: a call is tens of seconds),
the fill's pair kernels from dst_kernel_ms_mean (mean per launch x slabs per call), and the traffic model of the
rounds: the scan reads the active triangle once per round, sum over m of m^2 / 2 x 8 bytes.  Kernel times come from a
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

SHAPES = [   # name, records, sites, measure
    ("nj2k_raw", 2_000, 30_000, "raw"),
    ("nj10k_raw", 10_000, 30_000, "raw"),
    ("nj50k_raw", 50_000, 30_000, "raw"),
    ("nj50k_tn93", 50_000, 30_000, "tn93"),
]


def slab_count(n, bound=1 << 25):
    slabs, rb = 0, 0
    while rb < n - 1:
        pairs, re = 0, rb
        while re < n and (re == rb or pairs + (n - re - 1) <= bound):
            pairs += n - re - 1
            re += 1
        slabs += pairs > 0
        rb = re
    return slabs


def scan_bytes(n):
    """bytes the scans read: the active triangle of every round (m = n .. 4), 8 B per entry"""
    m = np.arange(4, n + 1, dtype=np.float64)
    return float(np.sum(m * (m - 1) / 2 * 8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--only", nargs="*", default=None)
    args = ap.parse_args()
    with da.Engine(0) as eng:
        for name, n, L, measure in SHAPES:
            if args.only and name not in args.only:
                continue
            eng.upload(0, synth.alignment(synth.SEED, n, L))
            if n < 50_000:
                eng.nj(measure)   # warm-up: code objects, slab scratch
            times, pair_totals, first = [], [], None
            for _ in range(args.steps):
                eng.kernel_ms_mean(reset=True)
                t0 = time.perf_counter()
                parent, length = eng.nj(measure)
                times.append((time.perf_counter() - t0) * 1e3)
                km = eng.kernel_ms_mean(reset=True)
                pair_totals.append(km["pair_ms"] * slab_count(n))
                if first is None:
                    first = (parent, length)
                else:
                    assert np.array_equal(first[0], parent) and np.array_equal(first[1].view(np.uint64), length.view(np.uint64))
            ms = float(np.median(times))
            sb = scan_bytes(n)
            print(json.dumps({
                "shape": name, "records": n, "sites": L, "measure": measure, "steps": args.steps,
                "ms_per_call": round(ms, 1), "ms_min": round(min(times), 1),
                "fill_pair_kernels_ms": round(float(np.median(pair_totals)), 1), "rounds": n - 3,
                "scan_bytes_model": sb, "model_ms_at_5TBps": round(sb / 5e12 * 1e3, 1),
                "effective_scan_TBps": round(sb / (ms * 1e-3) / 1e12, 2),
                "negative_lengths": int((length < 0).sum()), "path": eng.last_path(),
            }), flush=True)


if __name__ == "__main__":
    main()
